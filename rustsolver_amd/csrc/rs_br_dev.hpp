// rs_br_dev.hpp -- the device side of the best response (rs_br.hip, its only includer: every kernel is compiled in, and launched from, that one translation unit):
// the cell readers, the job and index structures the kernels take, and every kernel and body.
#pragma once

#include "rs_internal.hpp"
#include "rs_device.hpp"
#include "rs_eval.hpp"

#pragma clang fp contract(off)

namespace rs {

constexpr int kBrBlock = 256;

template <int DT> struct Elem;
template <> struct Elem<kDT_I32> {
    using val = int;
    static __device__ __forceinline__ val at(const void *base, size_t i) { return ((const int *)base)[i]; }
};
template <> struct Elem<kDT_F32> {
    using val = float;
    static __device__ __forceinline__ val at(const void *base, size_t i) { return ((const float *)base)[i]; }
};
template <> struct Elem<kDT_F16> {
    using val = float;
    static __device__ __forceinline__ val at(const void *base, size_t i) { return (float)((const _Float16 *)base)[i]; }
};

// Infoset::get_final_strategy (infoset.rs:104-123) of ONE lane of a node's strategy_sum rows [A][pitch]
template <int DT>
__device__ __forceinline__ void final_sigma(const void *ssum, size_t cell_off, uint32_t pitch, uint32_t n_actions, uint32_t lane,
                                            float (&sig)[RS_MAX_ACTIONS]) {
    using V = typename Elem<DT>::val;
    V r[RS_MAX_ACTIONS];
    float norm = 0.0f;
    for (uint32_t a = 0; a < n_actions; a++) {
        r[a] = Elem<DT>::at(ssum, cell_off + (size_t)a * pitch + lane);
        if (r[a] > (V)0) norm += (float)r[a];
    }
    const float uni = 1.0f / (float)n_actions;
    for (uint32_t a = 0; a < n_actions; a++) sig[a] = (norm > 0.0f) ? ((r[a] > (V)0) ? (float)r[a] / norm : 0.0f) : uni;
}

// Infoset::get_strategy (infoset.rs:83-102) of ONE lane of a node's REGRET rows: the same text over the other array (positive cells over their f32 sum in index order,
// uniform where none is positive; regret_match<A, float> of rs_device.hpp on f32 cells), so the readers above take the regret array where they are asked for the
// current strategy (RS_BR_CURRENT, the full-width sweep's reach)
// The full-width sweep's kernels call this form: unrolled to RS_MAX_ACTIONS with the action count as a predicate, so that r[] and sig[] stay registers (indexed by a
// run-time count they become scratch on gfx950); r[] hands the regret row back, entries from n_actions on are 0 / unused.
template <int DT>
__device__ __forceinline__ void current_sigma(const void *regrets, size_t cell_off, uint32_t pitch, uint32_t n_actions, uint32_t lane,
                                              typename Elem<DT>::val (&r)[RS_MAX_ACTIONS], float (&sig)[RS_MAX_ACTIONS]) {
    using V = typename Elem<DT>::val;
    float norm = 0.0f;
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++) {
        r[a] = (uint32_t)a < n_actions ? Elem<DT>::at(regrets, cell_off + (size_t)a * pitch + lane) : (V)0;
        if (r[a] > (V)0) norm += (float)r[a];
    }
    const float uni = 1.0f / (float)n_actions;
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++) sig[a] = (norm > 0.0f) ? ((r[a] > (V)0) ? (float)r[a] / norm : 0.0f) : uni;
}

struct BrNodeRow {   // one action node's strategy_sum block
    uint64_t cell_off;
    uint32_t pitch, n_actions;
};

// calc_br's reader: probabilites[0] of every action node (cfr.rs:669-672 with :677-679)
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_bucket0_final_strategy(const void *__restrict__ ssum, const BrNodeRow *__restrict__ rows, uint32_t n_nodes,
                                                                      float *__restrict__ out /*[n_nodes][RS_MAX_ACTIONS]*/) {
    const uint32_t n = blockIdx.x * kBrBlock + threadIdx.x;
    if (n >= n_nodes) return;
    const BrNodeRow row = rows[n];
    float sig[RS_MAX_ACTIONS];
    final_sigma<DT>(ssum, row.cell_off, row.pitch, row.n_actions, 0u, sig);
    for (uint32_t a = 0; a < RS_MAX_ACTIONS; a++) out[(size_t)n * RS_MAX_ACTIONS + a] = a < row.n_actions ? sig[a] : 0.0f;
}

// ---- best response, vector form ------------------------------------------------------------------------------------------
// score[h] of hole cards + the five board cards (the evaluator the showdown-sign kernel uses; only compared, cfr.rs:326-333)
__global__ __launch_bounds__(kBrBlock) void k_hand_scores(const uint8_t *__restrict__ hands /*[n][2]*/, uint32_t n, uint32_t b0, uint32_t b1, uint32_t b2,
                                                          uint32_t b3, uint32_t b4, uint32_t *__restrict__ score) {
    const uint32_t h = blockIdx.x * kBrBlock + threadIdx.x;
    if (h >= n) return;
    uint32_t m[4] = {0, 0, 0, 0};
    add_card(m, b0); add_card(m, b1); add_card(m, b2); add_card(m, b3); add_card(m, b4);
    add_card(m, hands[2 * h]);
    add_card(m, hands[2 * h + 1]);
    score[h] = evaluate_suits(m);
}

// terminal: v[hp] = pw[hp] * sum over the opponent's hands ho that share no card with hp, ascending, of q[ho] * u(hp, ho);
// u as the trainer's leaves (cfr.rs:314-348): UNCONTESTED -pot for the folder / +pot for the other, SHOWDOWN and ALLIN +-pot by score, 0 on a tie
__global__ __launch_bounds__(kBrBlock) void k_br_terminal(const uint64_t *__restrict__ mask_p, const uint32_t *__restrict__ score_p, const double *__restrict__ pw,
                                                          uint32_t n_p, const uint64_t *__restrict__ mask_o, const uint32_t *__restrict__ score_o,
                                                          const double *__restrict__ q, uint32_t n_o, int uncontested, double value, double *__restrict__ v) {
    const uint32_t hp = blockIdx.x * kBrBlock + threadIdx.x;
    if (hp >= n_p) return;
    const uint64_t mp = mask_p[hp];
    const uint32_t sp = score_p[hp];
    double acc = 0.0;
    for (uint32_t ho = 0; ho < n_o; ho++) {
        if (mp & mask_o[ho]) continue;
        const uint32_t so = score_o[ho];
        const double u = uncontested ? value : (sp > so ? value : (sp < so ? -value : 0.0));
        acc += q[ho] * u;
    }
    v[hp] = pw[hp] * acc;
}

// opponent node, on the way up: v[h] = v_0[h] + v_1[h] + ... in action order
__device__ __forceinline__ void br_sum_body(const double *__restrict__ vch /*[A][n_pad]*/, uint32_t n_actions, uint32_t n, uint32_t n_pad,
                                                     double *__restrict__ v) {
    const uint32_t h = blockIdx.x * kBrBlock + threadIdx.x;
    if (h >= n) return;
    double acc = 0.0;
    for (uint32_t a = 0; a < n_actions; a++) acc += vch[(size_t)a * n_pad + h];
    v[h] = acc;
}

// own node: one thread per info set (cluster).  RS_BR_MAX: the action with the largest value summed over the cluster's hands
// (ascending hand order; first maximum, strict < as cfr.rs:684-690) is played by every hand of the cluster; RS_BR_AVERAGE: sigma_bar.
template <int DT>
__device__ __forceinline__ void br_own_body(const void *__restrict__ ssum, BrNodeRow row, const uint32_t *__restrict__ start /*[n_clusters + 2]*/,
                                                     const uint32_t *__restrict__ order, uint32_t n_clusters, uint32_t n_pad, const double *__restrict__ vch,
                                                     int mode, double *__restrict__ v) {
    // lanes that are no deal at all (the hand uses a card of the run-out) are listed after the last cluster: worth 0, summed nowhere (x + 0.0 == x)
    for (uint32_t i = start[n_clusters] + blockIdx.x * kBrBlock + threadIdx.x; i < start[n_clusters + 1]; i += gridDim.x * kBrBlock) v[order[i]] = 0.0;
    const uint32_t c = blockIdx.x * kBrBlock + threadIdx.x;
    if (c >= n_clusters) return;
    const uint32_t lo = start[c], hi = start[c + 1];
    if (lo == hi) return;
    if (mode == RS_BR_MAX && hi - lo <= 8) {   // a river info set holds a handful of lanes: its lane ids once, then every (action, lane) value in flight together -- two round
                                               // trips instead of two per value; the additions in list order as below
        uint32_t idx[8];
#pragma unroll
        for (int k = 0; k < 8; k++) idx[k] = lo + k < hi ? order[lo + k] : order[lo];
        double s[RS_MAX_ACTIONS];
        uint32_t best = 0;
        for (uint32_t a = 0; a < row.n_actions; a++) {
            const double *va = vch + (size_t)a * n_pad;
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; k++) t[k] = va[idx[k]];
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (lo + k < hi) acc += t[k];
            s[a] = acc;
            if (a > 0 && s[best] < s[a]) best = a;
        }
        const double *vb = vch + (size_t)best * n_pad;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (lo + k < hi) v[idx[k]] = vb[idx[k]];
        return;
    }
    if (mode == RS_BR_MAX) {
        double s[RS_MAX_ACTIONS];
        for (uint32_t a = 0; a < row.n_actions; a++) {
            const double *va = vch + (size_t)a * n_pad;
            double acc = 0.0;
            uint32_t i = lo;
            for (; i + 8 <= hi; i += 8) {   // eight gathers in flight, the additions still one after the other in list order
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; k++) t[k] = va[order[i + k]];
#pragma unroll
                for (int k = 0; k < 8; k++) acc += t[k];
            }
            for (; i < hi; i++) acc += va[order[i]];
            s[a] = acc;
        }
        uint32_t best = 0;
        for (uint32_t a = 1; a < row.n_actions; a++)
            if (s[best] < s[a]) best = a;
        for (uint32_t i = lo; i < hi; i++) v[order[i]] = vch[(size_t)best * n_pad + order[i]];
    } else {
        float sig[RS_MAX_ACTIONS];
        final_sigma<DT>(ssum, row.cell_off, row.pitch, row.n_actions, c, sig);
        for (uint32_t i = lo; i < hi; i++) {
            const uint32_t h = order[i];
            double acc = 0.0;
            for (uint32_t a = 0; a < row.n_actions; a++) acc += (double)sig[a] * vch[(size_t)a * n_pad + h];
            v[h] = acc;
        }
    }
}

// the kernel's instantiation for the table's cell type
#define RS_BR_PICK(dtype_, K) ((dtype_) == RS_I32 ? K<kDT_I32> : ((dtype_) == RS_F32 ? K<kDT_F32> : K<kDT_F16>))

// ---- best response proper -----------------------------------------------------------------------------------------------
// Lanes are (run-out b, hand h), lane = b * n_hands + h: generate_hand (cfr.rs:100-143) completes the board to five cards before it draws the hands, every showdown
// compares seven-card hands on the FULL board and chance nodes pass through (cfr.rs:306-313), so every node carries vectors over all NB * n lanes; the betting round
// of a node only selects which cluster id a lane is looked up under.  A single-round game on a full board is NB = 1.

// seven-card scores of every lane (0 where the hand uses a card of the run-out: no such deal)
__global__ __launch_bounds__(kBrBlock) void k_lane_scores(const uint8_t *__restrict__ hands /*[n][2]*/, uint32_t n, const uint8_t *__restrict__ boards /*[NB][5]*/, uint32_t n_board0,
                                                          uint32_t NB, uint32_t *__restrict__ score) {
    const size_t lane = (size_t)blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= (size_t)NB * n) return;
    const uint32_t b = (uint32_t)(lane / n), h = (uint32_t)(lane - (size_t)b * n);
    const uint32_t c0 = hands[2 * h], c1 = hands[2 * h + 1];
    uint32_t m[4] = {0, 0, 0, 0};
    bool blocked = false;
    for (uint32_t i = 0; i < 5; i++) {
        const uint32_t c = boards[b * 5 + i];
        add_card(m, c);
        if (i >= n_board0 && (c == c0 || c == c1)) blocked = true;
    }
    add_card(m, c0);
    add_card(m, c1);
    score[lane] = blocked ? 0u : evaluate_suits(m);
}

// the deal distribution: w0[b, h0] = P(B) / (N0(B) * N1(B, h0)) (0 for a blocked lane or when no h1 fits)
__global__ __launch_bounds__(kBrBlock) void k_br_weights(const uint64_t *__restrict__ mask0, uint32_t n0, const uint64_t *__restrict__ mask1, uint32_t n1,
                                                         const uint64_t *__restrict__ bmask, const uint32_t *__restrict__ cnt0, uint32_t NB, double pb,
                                                         double *__restrict__ w0) {
    const size_t lane = (size_t)blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= (size_t)NB * n0) return;
    const uint32_t b = (uint32_t)(lane / n0), h = (uint32_t)(lane - (size_t)b * n0);
    const uint64_t mine = mask0[h], bm = bmask[b];
    if (mine & bm) {
        w0[lane] = 0.0;
        return;
    }
    uint32_t cnt1 = 0;
    for (uint32_t g = 0; g < n1; g++) cnt1 += ((mask1[g] & bm) == 0 && (mask1[g] & mine) == 0) ? 1u : 0u;
    w0[lane] = cnt1 ? pb / ((double)cnt0[b] * (double)cnt1) : 0.0;
}

// ---- weighted ranges (rs_range_weights): the same two lane rows from per-hand weights -------------------------------------------------------------------------------
// Z1(b, h0) = the sum of W1 over player 1's hands that avoid the run-out and h0, ascending from 0.0 (0.0 on a blocked lane).  One workgroup = up to 256 hands of player 0
// on one run-out; player 1's masks and weights are staged in LDS once (at most 1 326 x 16 bytes), as br_terminal_boards_body stages the opponent's side.
__global__ __launch_bounds__(kBrBlock) void k_br_weighted_z1(const uint64_t *__restrict__ mask0, uint32_t n0, const uint64_t *__restrict__ mask1,
                                                             const double *__restrict__ w1, uint32_t n1, const uint64_t *__restrict__ bmask, double *__restrict__ z1) {
    extern __shared__ unsigned char br_lds[];
    double *lw = (double *)br_lds;
    uint64_t *lm = (uint64_t *)(lw + n1);
    const uint32_t b = blockIdx.y;
    const uint64_t bm = bmask[b];
    for (uint32_t g = threadIdx.x; g < n1; g += kBrBlock) {
        lw[g] = w1[g];
        lm[g] = mask1[g];
    }
    __syncthreads();
    const uint32_t h = blockIdx.x * kBrBlock + threadIdx.x;
    if (h >= n0) return;
    const size_t lane = (size_t)b * n0 + h;
    const uint64_t mine = mask0[h];
    if (mine & bm) {
        z1[lane] = 0.0;
        return;
    }
    const uint64_t avoid = mine | bm;
    double acc = 0.0;
    for (uint32_t g = 0; g < n1; g++) {
        if (lm[g] & avoid) continue;
        acc += lw[g];
    }
    z1[lane] = acc;
}
// player 0's lane row from Z1, in place.  Sequential (z0 given): (pb * W0[h]) / (Z0(b) * Z1); joint (z0 null): W0[h] / Z, scale = Z; 0.0 where Z1 = 0 (blocked lanes are)
__global__ __launch_bounds__(kBrBlock) void k_br_weighted_lanes(const double *__restrict__ w0, uint32_t n0, const double *__restrict__ z0, uint32_t NB, double scale,
                                                                double *__restrict__ row) {
    const size_t lane = (size_t)blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= (size_t)NB * n0) return;
    const uint32_t b = (uint32_t)(lane / n0), h = (uint32_t)(lane - (size_t)b * n0);
    const double z1 = row[lane];
    double w = 0.0;
    if (z1 > 0.0) w = z0 ? (scale * w0[h]) / (z0[b] * z1) : w0[h] / scale;
    row[lane] = w;
}
// player 1's lane row: W1 on every run-out
__global__ __launch_bounds__(kBrBlock) void k_br_tile_weights(const double *__restrict__ w1, uint32_t n1, uint32_t NB, double *__restrict__ row) {
    const size_t lane = (size_t)blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= (size_t)NB * n1) return;
    row[lane] = w1[lane % n1];
}

// terminal: v[b, hp] = pw[b, hp] * sum over the opponent's hands ho of the SAME run-out that share no card with hp or the run-out, ascending, of q[b, ho] * u;
// u as the trainer's leaves (cfr.rs:314-348).  One workgroup = up to 256 hands of one run-out; the opponent's side of that run-out is staged in LDS.
// RAKED (rs_rake): a showdown's u is one of three payoffs -- value when the traverser wins, vt on a tie, vl when it loses; uncontested leaves keep
// their one scalar.  The unraked instantiations are the text they were.
template <bool RAKED>
__device__ __forceinline__ void br_terminal_boards_body(const uint64_t *__restrict__ mask_p, const uint32_t *__restrict__ score_p, const double *__restrict__ pw,
                                                                 uint32_t n_p, const uint64_t *__restrict__ mask_o, const uint32_t *__restrict__ score_o,
                                                                 const double *__restrict__ q, uint32_t n_o, const uint64_t *__restrict__ bmask, int uncontested,
                                                                 double value, double vt, double vl, double *__restrict__ v) {
    extern __shared__ unsigned char br_lds[];
    double *lq = (double *)br_lds;
    uint64_t *lm = (uint64_t *)(lq + n_o);
    uint32_t *ls = (uint32_t *)(lm + n_o);
    const uint32_t b = blockIdx.y;
    const uint64_t bm = bmask[b];
    for (uint32_t g = threadIdx.x; g < n_o; g += kBrBlock) {
        lq[g] = q[(size_t)b * n_o + g];
        lm[g] = mask_o[g];
        ls[g] = score_o[(size_t)b * n_o + g];
    }
    __syncthreads();
    const uint32_t hp = blockIdx.x * kBrBlock + threadIdx.x;
    if (hp >= n_p) return;
    const size_t lane = (size_t)b * n_p + hp;
    const uint64_t mp = mask_p[hp];
    if (mp & bm) {
        v[lane] = 0.0;
        return;
    }
    const uint32_t sp = score_p[lane];
    const uint64_t avoid = mp | bm;
    double acc = 0.0;
    for (uint32_t ho = 0; ho < n_o; ho++) {
        if (lm[ho] & avoid) continue;
        const uint32_t so = ls[ho];
        const double u = uncontested ? value : (sp > so ? value : (sp < so ? (RAKED ? vl : -value) : (RAKED ? vt : 0.0)));
        acc += lq[ho] * u;
    }
    v[lane] = pw[lane] * acc;
}

// ---- showdowns by rank order (RS_BR_SORTED): O(n log n) per run-out instead of the O(n^2) pair loop of cfr.rs:323-347 ------------------------------------------------
// For a showdown leaf, a traverser hand h collects value * (sum of q over the opponent hands it beats - sum over those that beat it), over the opponent hands that share
// no card with h or the run-out.  With the opponent's hands of a run-out SORTED by (score, index) -- the scores do not depend on the tree node, so the order and every
// position below are computed once per call (k_br_index) -- that is a difference of prefix sums P over the sorted order, corrected for the at most 2 x 51 opponent hands
// that hold one of h's cards through per-card prefix sums Pc:
//     win  = (P[nl - 1] - Pc[c0][kl0 - 1]) - Pc[c1][kl1 - 1]                     nl  = opponent hands with a smaller score, kl_t = those among the holders of h's card t
//     lose = ((T - P[nle - 1]) - (Tc[c0] - Pc[c0][kle0 - 1])) - (Tc[c1] - Pc[c1][kle1 - 1])      nle, kle_t = ... with a smaller or equal score; T, Tc = totals
//     acc  = value * (win - lose)
// (a hand holding BOTH cards is the same hand: equal score, in neither sum).  An uncontested leaf is value * (((T - Tc[c0]) - Tc[c1]) + q[same hand]).
// Every sum has ONE fixed order, which the oracle (orc_best_response_rounds, sorted mode) follows to the bit: P in 64 chunks of ceil(n / 64) consecutive sorted positions --
// chunk sums sequential from 0.0, chunk offsets sequential over the chunks, P[i] = offset + the sequential sum inside the chunk up to i -- and Pc sequential per card.
constexpr int kBrCardHolders = 51, kBrSortN = 2048;   // a card is held by at most 51 two-card hands; 1 326 hands at most, padded to a power of two for the sort
struct BrIndex {   // of one side as the OPPONENT (sorted hands, holders of every card) and of the other side's hands as the traverser (positions), all per run-out
    uint16_t *ord = nullptr;       // [NB][n_o] opponent hand at sorted position i (i < nv[b])
    uint16_t *nv = nullptr;        // [NB] opponent hands that avoid the run-out
    uint16_t *cl = nullptr;        // [NB][52][51] holders of card c in sorted order
    uint8_t *cc = nullptr;         // [NB][52] their number
    uint16_t *nl = nullptr, *nle = nullptr;   // [NB][n_p]
    uint8_t *kl = nullptr, *kle = nullptr;    // [NB][n_p][2]
    int16_t *same = nullptr;       // [n_p] the opponent's hand with the same two cards, -1 = none
};
__global__ __launch_bounds__(kBrBlock) void k_br_index(const uint8_t *__restrict__ hands_p, uint32_t n_p, const uint64_t *__restrict__ mask_p, const uint32_t *__restrict__ score_p,
                                                       const uint8_t *__restrict__ hands_o, uint32_t n_o, const uint64_t *__restrict__ mask_o,
                                                       const uint32_t *__restrict__ score_o, const uint64_t *__restrict__ bmask, BrIndex ix) {
    __shared__ unsigned long long key[kBrSortN];                 // (score << 16) | hand, ~0 = padding
    __shared__ uint16_t lcl[52][kBrCardHolders];
    __shared__ uint32_t lcs[52][kBrCardHolders];                 // the holders' scores
    __shared__ uint32_t lcc[52];
    __shared__ uint32_t lnv;
    const uint32_t b = blockIdx.x;
    const uint64_t bm = bmask[b];
    for (uint32_t i = threadIdx.x; i < (uint32_t)kBrSortN; i += kBrBlock)
        key[i] = (i < n_o && !(mask_o[i] & bm)) ? ((unsigned long long)score_o[(size_t)b * n_o + i] << 16 | i) : ~0ull;
    if (threadIdx.x == 0) lnv = 0;
    __syncthreads();
    for (uint32_t k = 2; k <= (uint32_t)kBrSortN; k <<= 1)       // bitonic sort, ascending
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < (uint32_t)kBrSortN; i += kBrBlock) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const unsigned long long x = key[i], y = key[l];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        key[i] = y;
                        key[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n_o; i += kBrBlock) {
        if (key[i] != ~0ull) {
            ix.ord[(size_t)b * n_o + i] = (uint16_t)(key[i] & 0xffffu);
            if (i + 1 == n_o || key[i + 1] == ~0ull) lnv = i + 1;
        } else ix.ord[(size_t)b * n_o + i] = 0;
    }
    __syncthreads();
    const uint32_t nv = lnv;
    if (threadIdx.x == 0) ix.nv[b] = (uint16_t)nv;
    if (threadIdx.x < 52) {                                      // the holders of card c, in sorted order
        const uint32_t c = threadIdx.x;
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < nv; ++i) {
            const uint32_t g = (uint32_t)(key[i] & 0xffffu);
            if (hands_o[2 * g] == c || hands_o[2 * g + 1] == c) {
                if (cnt < (uint32_t)kBrCardHolders) {
                    lcl[c][cnt] = (uint16_t)g;
                    lcs[c][cnt] = (uint32_t)(key[i] >> 16);
                    ix.cl[((size_t)b * 52 + c) * kBrCardHolders + cnt] = (uint16_t)g;
                }
                ++cnt;
            }
        }
        lcc[c] = min(cnt, (uint32_t)kBrCardHolders);
        ix.cc[(size_t)b * 52 + c] = (uint8_t)lcc[c];
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < n_p; h += kBrBlock) {     // where every traverser hand stands in the opponent's order
        const size_t lane = (size_t)b * n_p + h;
        if (mask_p[h] & bm) {
            ix.nl[lane] = ix.nle[lane] = 0;
            ix.kl[2 * lane] = ix.kl[2 * lane + 1] = ix.kle[2 * lane] = ix.kle[2 * lane + 1] = 0;
            continue;
        }
        const unsigned long long sp = score_p[lane];
        uint32_t lo = 0, hi = nv;                                // first position with score >= sp
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((key[mid] >> 16) < sp) lo = mid + 1; else hi = mid;
        }
        ix.nl[lane] = (uint16_t)lo;
        hi = nv;                                                 // first position with score > sp
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((key[mid] >> 16) <= sp) lo = mid + 1; else hi = mid;
        }
        ix.nle[lane] = (uint16_t)lo;
        for (int t = 0; t < 2; ++t) {
            const uint32_t c = hands_p[2 * h + t];
            uint32_t a = 0, e = 0;
            for (uint32_t j = 0; j < lcc[c]; ++j) {
                a += lcs[c][j] < sp ? 1u : 0u;
                e += lcs[c][j] <= sp ? 1u : 0u;
            }
            ix.kl[2 * lane + t] = (uint8_t)a;
            ix.kle[2 * lane + t] = (uint8_t)e;
        }
    }
}
// one workgroup per run-out: wave 0 builds P (chunked, see above) and the per-card prefixes in LDS, then all threads evaluate the traverser's hands
// RAKED: acc = ((value * win) + (vt * tie)) + (vl * lose), tie = (((LE - L) - (E0 - L0)) - (E1 - L1)) + q[same hand]: the opponent's hands of the traverser's score, less the
// holders of either of its cards among them -- the hand of the same two cards stands in both card lists, is taken off twice and comes back once
template <bool RAKED>
__device__ __forceinline__ void br_terminal_sorted_body(const uint8_t *__restrict__ hands_p, const uint64_t *__restrict__ mask_p, const double *__restrict__ pw,
                                                                 uint32_t n_p, const double *__restrict__ q, uint32_t n_o, const uint64_t *__restrict__ bmask, BrIndex ix,
                                                                 int uncontested, double value, double vt, double vl, double *__restrict__ v) {
    extern __shared__ unsigned char br_lds[];
    double *P = (double *)br_lds;                                // [n_o]
    double *Pc = P + n_o;                                        // [52][51]
    double *O = Pc + 52 * kBrCardHolders;                        // [65] chunk offsets, O[64] = total
    double *Q = O + 65;                                          // [n_o] the opponent's reach of this run-out: the scans below walk it in rank and card order
    const uint32_t b = blockIdx.x;
    const uint32_t nv = ix.nv[b];
    const double *__restrict__ qg = q + (size_t)b * n_o;
    for (uint32_t i = threadIdx.x; i < n_o; i += kBrBlock) Q[i] = qg[i];   // one coalesced pass; the dependent gathers then stay inside the LDS
    __syncthreads();
    const double *qb = Q;
    const uint16_t *__restrict__ ord = ix.ord + (size_t)b * n_o;
    const uint32_t len = (nv + 63u) / 64u;
    if (threadIdx.x < 64) {
        const uint32_t k = threadIdx.x, i0 = min(nv, k * len), i1 = min(nv, i0 + len);
        double sum = 0.0;
        for (uint32_t i = i0; i < i1; ++i) sum += qb[ord[i]];
        O[k] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                      // offsets: sequential over the chunks
        double run = 0.0;
        for (uint32_t k = 0; k < 64; ++k) {
            const double c = O[k];
            O[k] = run;
            run += c;
        }
        O[64] = run;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const uint32_t k = threadIdx.x, i0 = min(nv, k * len), i1 = min(nv, i0 + len);
        double local = 0.0;
        for (uint32_t i = i0; i < i1; ++i) {
            local += qb[ord[i]];
            P[i] = O[k] + local;
        }
    } else if (threadIdx.x < 64 + 52) {
        const uint32_t c = threadIdx.x - 64, cnt = ix.cc[(size_t)b * 52 + c];
        const uint16_t *__restrict__ cl = ix.cl + ((size_t)b * 52 + c) * kBrCardHolders;
        double run = 0.0;
        for (uint32_t j = 0; j < cnt; ++j) {
            run += qb[cl[j]];
            Pc[c * kBrCardHolders + j] = run;
        }
    }
    __syncthreads();
    const double T = O[64];
    const uint64_t bm = bmask[b];
    for (uint32_t h = threadIdx.x; h < n_p; h += kBrBlock) {
        const size_t lane = (size_t)b * n_p + h;
        if (mask_p[h] & bm) {
            v[lane] = 0.0;
            continue;
        }
        const uint32_t c0 = hands_p[2 * h], c1 = hands_p[2 * h + 1];
        const uint32_t n0 = ix.cc[(size_t)b * 52 + c0], n1 = ix.cc[(size_t)b * 52 + c1];
        const double T0 = n0 ? Pc[c0 * kBrCardHolders + n0 - 1] : 0.0, T1 = n1 ? Pc[c1 * kBrCardHolders + n1 - 1] : 0.0;
        double acc;
        if (uncontested) {
            const int sm = ix.same[h];
            acc = value * (((T - T0) - T1) + (sm >= 0 ? qb[sm] : 0.0));
        } else {
            const uint32_t nl = ix.nl[lane], nle = ix.nle[lane];
            const uint32_t a0 = ix.kl[2 * lane], a1 = ix.kl[2 * lane + 1], e0 = ix.kle[2 * lane], e1 = ix.kle[2 * lane + 1];
            const double L = nl ? P[nl - 1] : 0.0, LE = nle ? P[nle - 1] : 0.0;
            const double L0 = a0 ? Pc[c0 * kBrCardHolders + a0 - 1] : 0.0, L1 = a1 ? Pc[c1 * kBrCardHolders + a1 - 1] : 0.0;
            const double E0 = e0 ? Pc[c0 * kBrCardHolders + e0 - 1] : 0.0, E1 = e1 ? Pc[c1 * kBrCardHolders + e1 - 1] : 0.0;
            const double win = (L - L0) - L1;
            const double lose = ((T - LE) - (T0 - E0)) - (T1 - E1);
            if (RAKED) {
                const int sm = ix.same[h];
                const double tie = (((LE - L) - (E0 - L0)) - (E1 - L1)) + (sm >= 0 ? qb[sm] : 0.0);
                acc = ((value * win) + (vt * tie)) + (vl * lose);
            } else acc = value * (win - lose);
        }
        v[lane] = pw[lane] * acc;
    }
}

// one JOB per node and launch it takes part in: a grid row of the kind's kernel (the level plan: all nodes of one tree depth and kind in one launch; depth first: one row)
struct BrJob {
    BrNodeRow row;                 // action nodes: the node's strategy_sum block
    const uint32_t *cid;           // opponent node: the opponent's lane -> cluster of the node's round
    const uint32_t *start, *order; // own node: the lanes of every info set of the node's round
    const double *q;               // opponent node: the reach that comes in; terminal: the opponent's reach
    double *q_out;                 // opponent node: [A][n_pad] reach of its children
    const double *vch;             // action node: [A][n_pad] values of its children
    double *v;                     // where the node's own value goes (a slot of its parent's vch, or the root vector)
    uint32_t n_clusters, n_children;
    int uncontested, pad_;
    double value;
    const double *sum_src[RS_MAX_ACTIONS];   // own node by groups: child a is an opponent's node whose value is the sum of ITS children's rows (sum_n[a] of them, n_pad apart,
    uint32_t sum_n[RS_MAX_ACTIONS];          // from sum_src[a]) -- added up while the rows are staged instead of written by k_br_sum_jobs and read again; 0: child a's row is vch + a * n_pad
    const uint32_t *tord, *perm;   // own node by columns (k_br_own_cols_jobs): [kmax][n_sets] the k-th lane of the i-th info set, and which cluster that info set is
    uint32_t n_sets, kmax;
    double value_tie, value_lose;  // a showdown leaf of a raked run (rs_rake): what a tie and a loss pay the traverser; `value` is the win.  Read by the RAKED leaf kernels only
    // a report job (kBrReport) reads its node's vch and v, q = the traverser's own reach that came in, sum_src[0] = the node's mass row (written by the kBrMass job before it,
    // a leaf job: q = the opponent's reach at the node, uncontested, value 1.0), and writes q_out = the node's block of the call's output buffer
};
// The level plan's form (round 5): ONE workgroup per run-out takes every leaf of the tree in turn.  What the leaves share -- the run-out's rank order, the holders of every
// card, where each of the traverser's hands stands in that order, its weight -- is read ONCE (25 KB per run-out and side; the one-leaf kernel above read it again at each of the
// 1 073 leaves of the three-street tree: 45 of its 111 MB per launch), the order and the card lists into LDS, the per-hand positions into registers (at most kBrHandsPerThread
// hands per thread); per leaf the workgroup streams the opponent's reach of its run-out in and its hands' values out.  The sums are br_terminal_sorted_body's, order and all.
constexpr int kBrHandsPerThread = 6;   // 1 326 two-card hands at most, 256 threads
constexpr int kBrChunkMax = 21;        // ... in 64 chunks of the rank order
// (the kernel is compiled for four range sizes -- <HPT, CHUNK> = <1, 4> up to 256 combos, <2, 8> up to 512, <4, 16> up to 1 024, <6, 21> beyond: its scans are unrolled to those
// bounds, and at <6, 21> a 200-combo range paid for 1 326 -- until then small ranges kept a workgroup per (run-out, leaf), 2.5 M workgroups per traverser)
static_assert(kBrCardHolders == 3 * 17, "the card scans of k_br_terminal_sorted_loop run in three blocks of 17");
template <int HPT, int CHUNK, bool REG_IDX, bool RAKED>
__global__ __launch_bounds__(kBrBlock) void k_br_terminal_sorted_loop(const uint8_t *__restrict__ hands_p, const uint64_t *__restrict__ mask_p, const double *__restrict__ pw,
                                                                      uint32_t n_p, uint32_t n_o, const uint64_t *__restrict__ bmask, BrIndex ix,
                                                                      const BrJob *__restrict__ jobs, uint32_t n_jobs) {
    extern __shared__ unsigned char br_lds[];
    double *P = (double *)br_lds;                                // [n_o]
    double *Pc = P + n_o;                                        // [52][51]
    double *O = Pc + 52 * kBrCardHolders;                        // [65]
    double *Q = O + 65;                                          // [n_o]
    uint16_t *Lord = (uint16_t *)(Q + n_o);                      // [n_o rounded up to 4]
    uint16_t *Lcl = Lord + ((n_o + 3u) & ~3u);                   // [52][51]
    uint8_t *Lcc = (uint8_t *)(Lcl + 52 * kBrCardHolders);       // [52]
    const uint32_t b = blockIdx.x;
    const uint32_t nv = ix.nv[b];
    const uint64_t bm = bmask[b];
    for (uint32_t i = threadIdx.x; i < n_o; i += kBrBlock) Lord[i] = ix.ord[(size_t)b * n_o + i];
    for (uint32_t i = threadIdx.x; i < 52u * kBrCardHolders; i += kBrBlock) Lcl[i] = ix.cl[(size_t)b * 52 * kBrCardHolders + i];
    if (threadIdx.x < 52) Lcc[threadIdx.x] = ix.cc[(size_t)b * 52 + threadIdx.x];
    // this thread's hands: h = threadIdx.x + k * 256
    uint32_t hw0[HPT], hw1[HPT];     // hw0 = nl | nle << 16; hw1 = a0 | a1 << 8 | e0 << 16 | e1 << 24
    uint32_t hc[HPT];                              // c0 | c1 << 8 | live << 16 | (the opponent's hand of the same two cards + 1, or 0) << 17
    double hp[HPT];
#pragma unroll
    for (int k = 0; k < HPT; ++k) {
        const uint32_t h = threadIdx.x + (uint32_t)k * kBrBlock;
        hw0[k] = hw1[k] = hc[k] = 0;
        hp[k] = 0.0;
        if (h < n_p) {
            const size_t lane = (size_t)b * n_p + h;
            const bool live = !(mask_p[h] & bm);
            hc[k] = (uint32_t)hands_p[2 * h] | (uint32_t)hands_p[2 * h + 1] << 8 | (live ? 1u << 16 : 0u);
            if (live) {
                hw0[k] = (uint32_t)ix.nl[lane] | (uint32_t)ix.nle[lane] << 16;
                hw1[k] = (uint32_t)ix.kl[2 * lane] | (uint32_t)ix.kl[2 * lane + 1] << 8 | (uint32_t)ix.kle[2 * lane] << 16 | (uint32_t)ix.kle[2 * lane + 1] << 24;
                hc[k] |= (uint32_t)(ix.same[h] + 1) << 17;
                hp[k] = pw[lane];
            }
        }
    }
    const uint32_t len = (nv + 63u) / 64u;
    __syncthreads();
    // What the scans below walk is the same for every leaf, so it lives in registers: wave 0's lane k owns chunk k of the rank order (at most CHUNK positions), the first
    // 52 lanes of wave 1 a card's holders each.  Per leaf every value is then fetched from LDS in one go and added up in registers, in the body's order: a chunk's running sums,
    // the chunk offsets (one after the other over the lanes: readlane), P = offset + running sum; a card's running sums.  (The first version walked ord -> Q -> add -> store as
    // four dependent LDS operations per step, 51 steps for a card: 11.5 us per leaf and workgroup.)
    const uint32_t wave = threadIdx.x >> 6, wl = threadIdx.x & 63u;
    const uint32_t i0 = min(nv, wl * len), cnt0 = wave == 0 ? min(nv, i0 + len) - i0 : 0u;
    const uint32_t cardc = wl < 52u ? wl : 0u, cntc = (wave == 1 && wl < 52u) ? Lcc[cardc] : 0u;
    // REG_IDX (full ranges): the positions the scans read live in registers -- 72 of them, two workgroups per CU; from LDS at every leaf the kernel fits three workgroups
    // per CU at 168 registers and is slower (0.099 against 0.096 s per call).  The small-range forms (64-126 registers) read them from LDS: 200 combos 0.029 -> 0.026 s.
    uint32_t ordr[REG_IDX ? CHUNK : 1], clr[REG_IDX ? kBrCardHolders : 1];
    if (REG_IDX) {
#pragma unroll
        for (int k = 0; k < (REG_IDX ? CHUNK : 1); ++k) ordr[k] = (uint32_t)k < cnt0 ? Lord[i0 + k] : 0u;
#pragma unroll
        for (int k = 0; k < (REG_IDX ? kBrCardHolders : 1); ++k) clr[k] = (uint32_t)k < cntc ? Lcl[cardc * kBrCardHolders + k] : 0u;
    }
    uint32_t most_holders = 0;   // of any card in this run-out: a small range's card scans end after the first block of 17
    for (uint32_t c = 0; c < 52u; ++c) most_holders = max(most_holders, (uint32_t)Lcc[c]);
    // the opponent's reach of the NEXT leaf is fetched while this one is worked on: with two workgroups per CU nothing else hides a leaf's round trip to memory
    double qn[HPT];
    if (blockIdx.y < n_jobs) {
        const double *__restrict__ q0 = jobs[blockIdx.y].q + (size_t)b * n_o;
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const uint32_t i = threadIdx.x + (uint32_t)k * kBrBlock;
            qn[k] = i < n_o ? q0[i] : 0.0;
        }
    }
    for (uint32_t j = blockIdx.y; j < n_jobs; j += gridDim.y) {
        double *__restrict__ v = jobs[j].v;
        const int uncontested = jobs[j].uncontested;
        const double value = jobs[j].value;
        const double vt = RAKED ? jobs[j].value_tie : 0.0, vl = RAKED ? jobs[j].value_lose : 0.0;
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const uint32_t i = threadIdx.x + (uint32_t)k * kBrBlock;
            if (i < n_o) Q[i] = qn[k];
        }
        if (j + gridDim.y < n_jobs) {
            const double *__restrict__ q1 = jobs[j + gridDim.y].q + (size_t)b * n_o;
#pragma unroll
            for (int k = 0; k < HPT; ++k) {
                const uint32_t i = threadIdx.x + (uint32_t)k * kBrBlock;
                qn[k] = i < n_o ? q1[i] : 0.0;
            }
        }
        __syncthreads();
        if (wave == 0) {
            double t[CHUNK];
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) t[k] = Q[REG_IDX ? ordr[REG_IDX ? k : 0] : ((uint32_t)k < cnt0 ? Lord[i0 + k] : 0u)];
            double run = 0.0;
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) {
                if ((uint32_t)k < cnt0) run += t[k];
                t[k] = run;                                      // the chunk's running sum up to and including position k
            }
            const int s_lo = __double2loint(run), s_hi = __double2hiint(run);
            double off = 0.0, tot = 0.0;
            for (uint32_t k = 0; k < 64; ++k) {                  // offsets: sequential over the chunks
                const double c = __hiloint2double(__builtin_amdgcn_readlane(s_hi, (int)k), __builtin_amdgcn_readlane(s_lo, (int)k));
                if (wl == k) off = tot;
                tot += c;
            }
            if (!uncontested) {                                  // an uncontested leaf reads the totals only
#pragma unroll
                for (int k = 0; k < CHUNK; ++k)
                    if ((uint32_t)k < cnt0) P[i0 + k] = off + t[k];
            }
            if (wl == 0) O[64] = tot;
        } else if (wave == 1 && wl < 52u) {
            double run = 0.0;
#pragma unroll
            for (int k0 = 0; k0 < kBrCardHolders; k0 += 17) {
                if ((uint32_t)k0 >= most_holders) break;
                double t[17];
#pragma unroll
                for (int k = 0; k < 17; ++k) t[k] = Q[REG_IDX ? clr[REG_IDX ? k0 + k : 0] : ((uint32_t)(k0 + k) < cntc ? Lcl[cardc * kBrCardHolders + k0 + k] : 0u)];
#pragma unroll
                for (int k = 0; k < 17; ++k)
                    if ((uint32_t)(k0 + k) < cntc) {
                        run += t[k];
                        Pc[cardc * kBrCardHolders + k0 + k] = run;
                    }
            }
        }
        __syncthreads();
        const double T = O[64];
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const uint32_t h = threadIdx.x + (uint32_t)k * kBrBlock;
            if (h >= n_p) continue;
            const size_t lane = (size_t)b * n_p + h;
            if (!((hc[k] >> 16) & 1u)) {
                v[lane] = 0.0;
                continue;
            }
            const uint32_t c0 = hc[k] & 0xffu, c1 = (hc[k] >> 8) & 0xffu;
            const uint32_t n0 = Lcc[c0], n1 = Lcc[c1];
            const double T0 = n0 ? Pc[c0 * kBrCardHolders + n0 - 1] : 0.0, T1 = n1 ? Pc[c1 * kBrCardHolders + n1 - 1] : 0.0;
            double acc;
            if (uncontested) {
                acc = value * (((T - T0) - T1) + ((hc[k] >> 17) ? Q[(hc[k] >> 17) - 1u] : 0.0));
            } else {
                const uint32_t nl = hw0[k] & 0xffffu, nle = hw0[k] >> 16;
                const uint32_t a0 = hw1[k] & 0xffu, a1 = (hw1[k] >> 8) & 0xffu, e0 = (hw1[k] >> 16) & 0xffu, e1 = hw1[k] >> 24;
                const double L = nl ? P[nl - 1] : 0.0, LE = nle ? P[nle - 1] : 0.0;
                const double L0 = a0 ? Pc[c0 * kBrCardHolders + a0 - 1] : 0.0, L1 = a1 ? Pc[c1 * kBrCardHolders + a1 - 1] : 0.0;
                const double E0 = e0 ? Pc[c0 * kBrCardHolders + e0 - 1] : 0.0, E1 = e1 ? Pc[c1 * kBrCardHolders + e1 - 1] : 0.0;
                const double win = (L - L0) - L1;
                const double lose = ((T - LE) - (T0 - E0)) - (T1 - E1);
                if (RAKED) {
                    const double tie = (((LE - L) - (E0 - L0)) - (E1 - L1)) + ((hc[k] >> 17) ? Q[(hc[k] >> 17) - 1u] : 0.0);
                    acc = ((value * win) + (vt * tie)) + (vl * lose);
                } else acc = value * (win - lose);
            }
            v[lane] = hp[k] * acc;
        }
        __syncthreads();                                         // Q, P, Pc, O are the next leaf's
    }
}

// the same with one WAVE per info set, for rounds whose info sets hold many lanes (a flop info set of the 1 176-combo game: 3 800 of the 2.8 M lanes -- one thread per info set
// left three workgroups walking 3 800 dependent gathers each, 13 ms per node).  The lanes of the wave fetch 64 list entries at a time; the additions still run one after the
// other in list order (every lane adds the 64 values in the same order, read from its neighbours' registers), so the sums keep the oracle's bits.
template <int DT>
__device__ __forceinline__ void br_own_wave_body(const void *__restrict__ ssum, BrNodeRow row, const uint32_t *__restrict__ start /*[n_clusters + 2]*/,
                                                          const uint32_t *__restrict__ order, uint32_t n_clusters, uint32_t n_pad, const double *__restrict__ vch,
                                                          int mode, double *__restrict__ v) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * kBrBlock + threadIdx.x) >> 6, n_waves = gridDim.x * (kBrBlock >> 6);
    for (uint32_t i = start[n_clusters] + blockIdx.x * kBrBlock + threadIdx.x; i < start[n_clusters + 1]; i += gridDim.x * kBrBlock) v[order[i]] = 0.0;
    for (uint32_t c = wave; c < n_clusters; c += n_waves) {
        const uint32_t lo = start[c], hi = start[c + 1];
        if (lo == hi) continue;
        if (mode == RS_BR_MAX) {
            double s[RS_MAX_ACTIONS];
            for (uint32_t a = 0; a < row.n_actions; a++) {
                const double *va = vch + (size_t)a * n_pad;
                double acc = 0.0;
                for (uint32_t i = lo; i < hi; i += 64) {
                    const uint32_t cnt = min(64u, hi - i);
                    const double t = lane < cnt ? va[order[i + lane]] : 0.0;
                    const int t_lo = __double2loint(t), t_hi = __double2hiint(t);
                    for (uint32_t k = 0; k < cnt; ++k)   // cnt is wave-uniform
                        acc += __hiloint2double(__builtin_amdgcn_readlane(t_hi, (int)k), __builtin_amdgcn_readlane(t_lo, (int)k));
                }
                s[a] = acc;
            }
            uint32_t best = 0;
            for (uint32_t a = 1; a < row.n_actions; a++)
                if (s[best] < s[a]) best = a;
            for (uint32_t i = lo + lane; i < hi; i += 64) v[order[i]] = vch[(size_t)best * n_pad + order[i]];
        } else {
            float sig[RS_MAX_ACTIONS];
            final_sigma<DT>(ssum, row.cell_off, row.pitch, row.n_actions, c, sig);
            for (uint32_t i = lo + lane; i < hi; i += 64) {
                const uint32_t h = order[i];
                double acc = 0.0;
                for (uint32_t a = 0; a < row.n_actions; a++) acc += (double)sig[a] * vch[(size_t)a * n_pad + h];
                v[h] = acc;
            }
        }
    }
}


// ---- own nodes by groups of run-outs (level plan, RS_BR_MAX) ------------------------------------------------------------------------------------------------------
// A lossless river abstraction puts four lanes in an info set, each in a run-out of its own (the two orders of turn and river card, the swap of the two suits the flop does
// not hold): a thread per info set (br_own_body) fetches every 8-byte child value as a cache line of its own and moves nine times its algorithmic bytes (profiles/r05_br.md:
// 461 GB per call at the HBM roofline).  But the info sets of such a round stay within FEW run-outs: the run-outs fall into components (run-outs that share an info set) of
// two, four or eight run-outs there.  br_prepare packs components into groups of `cap` run-outs; a workgroup takes one group: the group's rows of a child's values come in
// whole (9 KB of consecutive doubles per run-out) into LDS, the info sets add up from LDS in br_own_body's order (same sums, same bits) and note the action that leads; each
// thread keeps the leader's value of the lanes it fetched and writes them out as whole rows.  Each child row is read once, the node's row written once.
struct BrGroups {
    const uint32_t *runouts;   // [n_groups][cap]: the group's run-outs (0xffffffff: none)
    const uint32_t *cstart;    // [n_groups + 1]: the group's info sets, as positions in lstart
    const uint32_t *lstart;    // [info sets + 1]: an info set's lanes in llane
    const uint16_t *llane;     // slot * n_hands + hand, in the order of BrSide::d_order (ascending lane)
    const uint16_t *lane_set;  // [n_groups][cap * n_hands]: the lane's info set within its group (0xffff: none -- the hand holds a card of the run-out, or no run-out in the slot)
    const uint32_t *set_cluster;   // [info sets]: the cluster id (k_br_opp_reach_grouped_jobs looks the strategy-sum rows up once per info set)
    uint32_t n_groups, cap, n_hands, max_sets;
};
constexpr uint32_t kBrGroupLanes = 5400;   // lanes a group is packed up to (cap = kBrGroupLanes / n_hands run-outs, at least the largest component): four run-outs of 1 176-1 326 hands
constexpr int kBrGroupBlock = 1024;    // one workgroup per CU at eight run-outs of 1 176 hands (75 KB of staged values + 26 KB of sums and leaders): sixteen waves of it
constexpr int kBrGroupPerThread = 11;  // cap * n_hands <= 11 264 values per row set (eight run-outs of 1 326 hands)
__global__ __launch_bounds__(kBrGroupBlock) void k_br_own_grouped_jobs(const BrJob *__restrict__ jobs, BrGroups g, uint32_t n_pad) {
    extern __shared__ double br_group_lds[];
    const BrJob j = jobs[blockIdx.y];
    const uint32_t grp = blockIdx.x, tid = threadIdx.x, GH = g.cap * g.n_hands;
    double *stage = br_group_lds, *bestv = stage + GH;
    uint32_t *besta = reinterpret_cast<uint32_t *>(bestv + g.max_sets);
    uint32_t goff[kBrGroupPerThread];   // the thread's values of a row set: global lane, or none
    uint32_t setof[kBrGroupPerThread];
    double outv[kBrGroupPerThread], regs[kBrGroupPerThread];
#pragma unroll
    for (int k = 0; k < kBrGroupPerThread; k++) {
        const uint32_t e = tid + uint32_t(k) * kBrGroupBlock;
        goff[k] = 0xffffffffu;
        setof[k] = 0xffffu;
        outv[k] = 0.0;   // a lane in no info set (its hand holds a card of the run-out) is worth 0
        if (e < GH) {
            const uint32_t slot = e / g.n_hands, ro = g.runouts[(size_t)grp * g.cap + slot];
            if (ro != 0xffffffffu) {
                goff[k] = ro * g.n_hands + (e - slot * g.n_hands);
                setof[k] = g.lane_set[(size_t)grp * GH + e];
            }
        }
    }
    const uint32_t c_lo = g.cstart[grp], c_hi = g.cstart[grp + 1];
    // child a's values of this thread's lanes: the child's row, or -- the child an opponent's node -- the sum of its children's rows in action order (br_sum_body's additions)
    const BrJob *__restrict__ jp = jobs + blockIdx.y;   // (sum_src / sum_n are indexed by the action: read where they lie, not from the by-value copy)
    auto fetch = [&](uint32_t a) {
        const uint32_t ns = jp->sum_n[a];
        if (ns == 0) {
            const double *va = j.vch + (size_t)a * n_pad;
#pragma unroll
            for (int k = 0; k < kBrGroupPerThread; k++) regs[k] = goff[k] != 0xffffffffu ? va[goff[k]] : 0.0;
            return;
        }
#pragma unroll
        for (int k = 0; k < kBrGroupPerThread; k++) regs[k] = 0.0;
        const double *src = jp->sum_src[a];
        for (uint32_t c = 0; c < ns; c++) {
            const double *vc = src + (size_t)c * n_pad;
#pragma unroll
            for (int k = 0; k < kBrGroupPerThread; k++) regs[k] += goff[k] != 0xffffffffu ? vc[goff[k]] : 0.0;
        }
    };
    fetch(0);
    for (uint32_t a = 0; a < j.n_children; a++) {
#pragma unroll
        for (int k = 0; k < kBrGroupPerThread; k++) {
            const uint32_t e = tid + uint32_t(k) * kBrGroupBlock;
            if (e < GH) stage[e] = regs[k];
        }
        __syncthreads();
        if (a + 1 < j.n_children) fetch(a + 1);   // the next child's rows are on their way while this one's info sets add up
        for (uint32_t c = c_lo + tid; c < c_hi; c += kBrGroupBlock) {
            const uint32_t lo = g.lstart[c], hi = g.lstart[c + 1];
            double acc = 0.0;
            for (uint32_t i = lo; i < hi; i++) acc += stage[g.llane[i]];   // list order: br_own_body's sum
            if (a == 0 || bestv[c - c_lo] < acc) {                          // first maximum, strict < (cfr.rs:684-690)
                bestv[c - c_lo] = acc;
                besta[c - c_lo] = a;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBrGroupPerThread; k++)
            if (setof[k] != 0xffffu && besta[setof[k]] == a) outv[k] = stage[tid + uint32_t(k) * kBrGroupBlock];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kBrGroupPerThread; k++)
        if (goff[k] != 0xffffffffu) j.v[goff[k]] = outv[k];
}

// The opponent's reach through the same groups: sigma_bar of an info set is computed ONCE (a lane-parallel kernel gathers the strategy-sum rows for each of its 4.3 lanes)
// into LDS; the group's lanes then stream through: q in, A products out, whole rows.  Lanes in no info set take cluster 0's strategy, as k_br_opp_reach_jobs has it (their
// reach is never looked at: the leaves skip hands that hold a card of the run-out).
template <int DT>
__global__ __launch_bounds__(kBrGroupBlock) void k_br_opp_reach_grouped_jobs(const void *__restrict__ ssum, const BrJob *__restrict__ jobs, BrGroups g, uint32_t n_pad) {
    extern __shared__ double br_group_lds[];
    float *sg = reinterpret_cast<float *>(br_group_lds);   // [A][max_sets + 1]
    const BrJob j = jobs[blockIdx.y];
    // workgroups go round the eight XCDs in turn: XCD x takes the groups [x n/8, (x+1) n/8) in order, so that neighbouring groups -- whose info sets are neighbours in the
    // strategy-sum rows (br_prepare packs the components in the order of their cluster ids) -- meet in one L2 at about the same time
    const uint32_t per_xcd = (g.n_groups + 7u) / 8u, grp = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (grp >= g.n_groups || (blockIdx.x >> 3) >= per_xcd) return;
    const uint32_t tid = threadIdx.x, GH = g.cap * g.n_hands, A = j.row.n_actions, pitch = g.max_sets + 1;
    const uint32_t c_lo = g.cstart[grp], n_sets = g.cstart[grp + 1] - c_lo;
    for (uint32_t k = tid; k <= n_sets; k += kBrGroupBlock) {
        float sig[RS_MAX_ACTIONS];
        final_sigma<DT>(ssum, j.row.cell_off, j.row.pitch, A, k < n_sets ? g.set_cluster[c_lo + k] : 0u, sig);
        const uint32_t at = k < n_sets ? k : g.max_sets;
        for (uint32_t a = 0; a < A; a++) sg[a * pitch + at] = sig[a];
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t e = tid; e < GH; e += kBrGroupBlock) {
        const uint32_t slot = e / g.n_hands, ro = g.runouts[(size_t)grp * g.cap + slot];
        if (ro == 0xffffffffu) continue;
        const uint32_t h = ro * g.n_hands + (e - slot * g.n_hands), set = g.lane_set[(size_t)grp * GH + e];
        const uint32_t at = set != 0xffffu ? set : g.max_sets;
        const double qh = j.q[h];
        for (uint32_t a = 0; a < A; a++) j.q_out[(size_t)a * n_pad + h] = qh * (double)sg[a * pitch + at];
    }
}

// ---- own nodes by columns (level plan) ---------------------------------------------------------------------------------------------------------------------------
// A lossless turn abstraction puts ~92 lanes in an info set: one hand under one turn card, every river card (and the suit-swapped twin).  A wave per info set
// (br_own_wave_body) reads 64 lanes of 64 run-outs per step: every 8-byte value a cache line of its own, eight times the algorithmic bytes (profiles/r05_br.md).  Here a THREAD
// takes an info set, and the info sets are ordered by their first lane: neighbouring threads hold neighbouring hands under the same turn card, so the k-th lanes of a wave's
// info sets lie side by side in one run-out's row (where a hand holds a river card its list is one entry ahead of its neighbours': two rows).  The lane lists come
// transposed ([k][info set]) so that the indices load coalesced too.  The sums run down each list in order: br_own_body's, and the wave kernel's, bits.
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_own_cols_jobs(const void *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n_pad, int mode) {
    const BrJob j = jobs[blockIdx.y];
    for (uint32_t i = j.start[j.n_clusters] + blockIdx.x * kBrBlock + threadIdx.x; i < j.start[j.n_clusters + 1]; i += gridDim.x * kBrBlock) j.v[j.order[i]] = 0.0;
    const uint32_t i = blockIdx.x * kBrBlock + threadIdx.x;
    if (i >= j.n_sets) return;
    const uint32_t *__restrict__ col = j.tord + i;
    const uint32_t A = j.row.n_actions;
    if (mode == RS_BR_MAX) {
        double s_best = 0.0;
        uint32_t best = 0;
        for (uint32_t a = 0; a < A; a++) {
            const double *va = j.vch + (size_t)a * n_pad;
            double acc = 0.0;
            for (uint32_t k = 0; k < j.kmax; k += 8) {   // eight gathers in flight (sixteen: no faster), the additions one after the other in list order
                uint32_t idx[8];
                double t[8];
#pragma unroll
                for (int q = 0; q < 8; q++) idx[q] = k + q < j.kmax ? col[(size_t)(k + q) * j.n_sets] : 0xffffffffu;
#pragma unroll
                for (int q = 0; q < 8; q++) t[q] = idx[q] != 0xffffffffu ? va[idx[q]] : 0.0;
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (idx[q] != 0xffffffffu) acc += t[q];
            }
            if (a == 0 || s_best < acc) s_best = acc, best = a;   // first maximum, strict < (cfr.rs:684-690)
        }
        const double *vb = j.vch + (size_t)best * n_pad;
        for (uint32_t k = 0; k < j.kmax; k += 8) {   // the winner's values: eight lanes' indices, then their values, then the stores
            uint32_t idx[8];
            double t[8];
#pragma unroll
            for (int q = 0; q < 8; q++) idx[q] = k + q < j.kmax ? col[(size_t)(k + q) * j.n_sets] : 0xffffffffu;
#pragma unroll
            for (int q = 0; q < 8; q++) t[q] = idx[q] != 0xffffffffu ? vb[idx[q]] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (idx[q] != 0xffffffffu) j.v[idx[q]] = t[q];
        }
    } else {
        float sig[RS_MAX_ACTIONS];
        final_sigma<DT>(ssum, j.row.cell_off, j.row.pitch, A, j.perm[i], sig);
        for (uint32_t k = 0; k < j.kmax; k++) {
            const uint32_t h = col[(size_t)k * j.n_sets];
            if (h == 0xffffffffu) continue;
            double acc = 0.0;
            for (uint32_t a = 0; a < A; a++) acc += (double)sig[a] * j.vch[(size_t)a * n_pad + h];
            j.v[h] = acc;
        }
    }
}

// ---- own nodes in the real game (RS_BR_MAX | RS_BR_REAL) ---------------------------------------------------------------------------------------------------------
// The traverser sees its own two cards: an info set of round r is (prefix of round r, hand), and its lanes are hand h under the run-outs [f * pp, (f + 1) * pp) of the
// prefix (pp = per_prefix[r]; enumerate_runouts puts the first new card most significant) -- lane (f * pp + k) * n_hands + h, an arithmetic progression.  No lists, no
// cluster ids: a thread takes a (prefix, hand) pair, neighbouring threads neighbouring hands, so run-out k of a wave's info sets is ONE stretch of a row.  Lanes whose hand
// holds a card of the run-out are no deal: not added, worth 0.  The sums run down the run-outs in ascending order from 0.0 and the first maximum under strict < wins --
// what br_own_body computes when every (prefix, hand) pair is a cluster of its own, bit for bit.
// A child that is an opponent's node (level plan) is not summed by k_br_sum_jobs first: its children's rows are added up here in action order from 0.0 (br_sum_body's
// additions) as they are loaded, as k_br_own_grouped_jobs does.
struct BrRealChild {
    const double *row;   // ns == 0: the child's row; else the first of ns rows, n_pad apart, whose sum in order is the child's row
    uint32_t ns;
};
__device__ __forceinline__ BrRealChild br_real_child(const double *__restrict__ vch, const BrJob *__restrict__ jp, uint32_t a, uint32_t n_pad) {
    if (jp->sum_n[a]) return {jp->sum_src[a], jp->sum_n[a]};   // (read where they lie: indexed by the action)
    return {vch + (size_t)a * n_pad, 0u};
}
template <int N>
__device__ __forceinline__ void br_real_load(BrRealChild ch, uint32_t n_pad, const uint32_t (&lane)[N], double (&t)[N]) {
    if (ch.ns == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) t[q] = ch.row[lane[q]];
        return;
    }
#pragma unroll
    for (int q = 0; q < N; q++) t[q] = 0.0;
    for (uint32_t c = 0; c < ch.ns; c++) {
        const double *vc = ch.row + (size_t)c * n_pad;
#pragma unroll
        for (int q = 0; q < N; q++) t[q] += vc[lane[q]];
    }
}
// the last round (pp == 1): an info set is a single lane, the node an element-wise first maximum over its children's rows -- every child row read once, the node's row
// written once, all of it whole rows
__device__ __forceinline__ void br_own_real_last_body(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n, uint32_t n_pad,
                                                      uint32_t n_actions, const double *__restrict__ vch, const BrJob *__restrict__ jp, double *__restrict__ v) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    const uint32_t b = lane / n_hands, h = lane - b * n_hands;
    if (mask_p[h] & bmask[b]) {
        v[lane] = 0.0;
        return;
    }
    const uint32_t at[1] = {lane};
    double t[RS_MAX_ACTIONS][1];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)   // every child's value on its way before the first comparison
        if ((uint32_t)a < n_actions) br_real_load<1>(br_real_child(vch, jp, (uint32_t)a, n_pad), n_pad, at, t[a]);
    double best = t[0][0];
#pragma unroll
    for (int a = 1; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < n_actions && best < t[a][0]) best = t[a][0];   // first maximum, strict < (cfr.rs:684-690); the sum of one lane compares as the lane
    v[lane] = best;
}
// earlier rounds (pp = 48 or 2 352 run-outs per info set): a workgroup takes 64 neighbouring (prefix, hand) pairs, and its four waves share the ACTIONS (wave w adds up
// actions w, w + 4, ...): each action's additions stay sequential down the run-outs, eight loads in flight as in k_br_own_cols_jobs, and a flop node of n_hands info sets
// gets four times the waves a thread per info set would give it.  The sums meet in 4 KB of LDS, every thread picks its pair's leader, and the waves share the run-outs of
// the write-back in blocks of eight.  (A thread per (info set, action) with the choice made through LDS: the split the chain of 2 352 dependent additions asks for; the
// lanes themselves never pass through LDS.)
constexpr int kBrRealPairs = 64, kBrRealWaves = kBrBlock / 64, kBrRealFlight = 8;
__device__ __forceinline__ void br_own_real_cols_body(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n_pairs, uint32_t pp,
                                                      uint32_t n_pad, uint32_t n_actions, const double *__restrict__ vch, const BrJob *__restrict__ jp, double *__restrict__ v) {
    __shared__ double sums[RS_MAX_ACTIONS][kBrRealPairs];
    const uint32_t x = threadIdx.x & 63u, w = threadIdx.x >> 6, pair = blockIdx.x * kBrRealPairs + x;
    const bool valid = pair < n_pairs;
    const uint32_t f = valid ? pair / n_hands : 0u, h = valid ? pair - f * n_hands : 0u;
    const uint64_t mine = mask_p[h];
    const uint64_t *__restrict__ bm = bmask + (size_t)f * pp;
    const uint32_t lane0 = f * pp * n_hands + h;   // run-out k of the pair: lane0 + k * n_hands (below n < 2^31)
    if (valid)
        for (uint32_t a = w; a < n_actions; a += kBrRealWaves) {
            const BrRealChild ch = br_real_child(vch, jp, a, n_pad);
            double acc = 0.0;
            for (uint32_t k = 0; k < pp; k += kBrRealFlight) {
                uint32_t lane[kBrRealFlight];
                bool deal[kBrRealFlight];
                double t[kBrRealFlight];
#pragma unroll
                for (int q = 0; q < kBrRealFlight; q++) {
                    const uint32_t kk = min(k + q, pp - 1);
                    lane[q] = lane0 + kk * n_hands;
                    deal[q] = k + q < pp && !(mine & bm[kk]);
                }
                br_real_load<kBrRealFlight>(ch, n_pad, lane, t);
#pragma unroll
                for (int q = 0; q < kBrRealFlight; q++)
                    if (deal[q]) acc += t[q];   // ascending run-outs, one after the other
            }
            sums[a][x] = acc;
        }
    __syncthreads();
    if (!valid) return;
    uint32_t best = 0;
    for (uint32_t a = 1; a < n_actions; a++)
        if (sums[best][x] < sums[a][x]) best = a;   // first maximum, strict < (cfr.rs:684-690)
    const BrRealChild ch = br_real_child(vch, jp, best, n_pad);
    for (uint32_t k = w * kBrRealFlight; k < pp; k += kBrRealWaves * kBrRealFlight) {
        uint32_t lane[kBrRealFlight];
        bool deal[kBrRealFlight];
        double t[kBrRealFlight];
#pragma unroll
        for (int q = 0; q < kBrRealFlight; q++) {
            const uint32_t kk = min(k + q, pp - 1);
            lane[q] = lane0 + kk * n_hands;
            deal[q] = !(mine & bm[kk]);
        }
        br_real_load<kBrRealFlight>(ch, n_pad, lane, t);
#pragma unroll
        for (int q = 0; q < kBrRealFlight; q++)
            if (k + q < pp) v[lane[q]] = deal[q] ? t[q] : 0.0;
    }
}
__global__ __launch_bounds__(kBrBlock) void k_br_own_real_last_jobs(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n,
                                                                    uint32_t n_pad, const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_own_real_last_body(mask_p, bmask, n_hands, n, n_pad, jp->n_children, jp->vch, jp, jp->v);
}
__global__ __launch_bounds__(kBrBlock) void k_br_own_real_cols_jobs(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n_pairs,
                                                                    uint32_t pp, uint32_t n_pad, const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_own_real_cols_body(mask_p, bmask, n_hands, n_pairs, pp, n_pad, jp->n_children, jp->vch, jp, jp->v);
}

// ---- the kernels: one JOB per node and grid row, a wrapper that hands the job's fields to the kind's body.  The level plan launches all nodes of one tree depth and kind
// at once, the depth-first walk one row of the same table (k_br_own_wave apart): BrRun::launch is the one launch path. -----------------------------------------------------
// opponent node: q_a[h] = q[h] * sigma_bar(cluster(h), a) for every action (cfr.rs:585's reach product, over the whole range at once)
// The strategy-sum rows are gathered by cluster id, and a lossless abstraction numbers its clusters hand by hand: workgroups go round the eight XCDs in turn, so
// workgroup x takes hands of slice x % 8 only (every run-out of them) -- an XCD's L2 then sees an eighth (with the suit-swapped twins: a quarter) of the node's rows instead of
// all of them (the river's 7.7 MB per node against 4 MB of L2: 250 MB fetched per node, profiles/r05_br.md).  gridDim.x = 8 * ceil(run-outs * ceil(n_hands / 8) / kBrBlock).
// The thread's lane h of the n = run-outs * n_hands; false: it has none (the slice is empty -- fewer than eight hands -- or the thread is past its end).
__device__ __forceinline__ bool br_xcd_sliced_lane(uint32_t n, uint32_t n_hands, uint32_t &h) {
    const uint32_t xcd = blockIdx.x & 7u, w = blockIdx.x >> 3, per = (n_hands + 7u) / 8u, lo = xcd * per;
    if (lo >= n_hands) return false;
    const uint32_t hs = min(per, n_hands - lo), idx = w * kBrBlock + threadIdx.x, b = idx / hs;
    h = b * n_hands + lo + (idx - b * hs);
    return h < n && b < n / n_hands;
}
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_opp_reach_jobs(const void *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n, uint32_t n_pad, uint32_t n_hands) {
    const BrJob j = jobs[blockIdx.y];
    uint32_t h;
    if (!br_xcd_sliced_lane(n, n_hands, h)) return;
    float sig[RS_MAX_ACTIONS];
    final_sigma<DT>(ssum, j.row.cell_off, j.row.pitch, j.row.n_actions, j.cid[h], sig);
    const double qh = j.q[h];
    for (uint32_t a = 0; a < j.row.n_actions; a++) j.q_out[(size_t)a * n_pad + h] = qh * (double)sig[a];
}
__global__ __launch_bounds__(kBrBlock) void k_br_sum_jobs(const BrJob *__restrict__ jobs, uint32_t n, uint32_t n_pad) {
    const BrJob j = jobs[blockIdx.y];
    br_sum_body(j.vch, j.n_children, n, n_pad, j.v);
}
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_own_jobs(const void *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n_pad, int mode) {
    const BrJob j = jobs[blockIdx.y];
    br_own_body<DT>(ssum, j.row, j.start, j.order, j.n_clusters, n_pad, j.vch, mode, j.v);
}
// The one kind with a one-node entry beside its job entry, the node's fields as kernel arguments: the depth-first walk launches it, because the i32 instantiation ran 8 %
// longer per launch from a job row there (100.3 against 92.5 us at 200 combos a side, profiles/br_launcher.md)
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_own_wave(const void *__restrict__ ssum, BrNodeRow row, const uint32_t *__restrict__ start, const uint32_t *__restrict__ order,
                                                          uint32_t n_clusters, uint32_t n_pad, const double *__restrict__ vch, int mode, double *__restrict__ v) {
    br_own_wave_body<DT>(ssum, row, start, order, n_clusters, n_pad, vch, mode, v);
}
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_own_wave_jobs(const void *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n_pad, int mode) {
    const BrJob j = jobs[blockIdx.y];
    br_own_wave_body<DT>(ssum, j.row, j.start, j.order, j.n_clusters, n_pad, j.vch, mode, j.v);
}
template <bool RAKED>
__global__ __launch_bounds__(kBrBlock) void k_br_terminal_sorted_jobs(const uint8_t *__restrict__ hands_p, const uint64_t *__restrict__ mask_p, const double *__restrict__ pw,
                                                                      uint32_t n_p, uint32_t n_o, const uint64_t *__restrict__ bmask, BrIndex ix,
                                                                      const BrJob *__restrict__ jobs) {
    const BrJob j = jobs[blockIdx.y];
    br_terminal_sorted_body<RAKED>(hands_p, mask_p, pw, n_p, j.q, n_o, bmask, ix, j.uncontested, j.value, RAKED ? j.value_tie : 0.0, RAKED ? j.value_lose : 0.0, j.v);
}
template <bool RAKED>
__global__ __launch_bounds__(kBrBlock) void k_br_terminal_boards_jobs(const uint64_t *__restrict__ mask_p, const uint32_t *__restrict__ score_p, const double *__restrict__ pw,
                                                                      uint32_t n_p, const uint64_t *__restrict__ mask_o, const uint32_t *__restrict__ score_o, uint32_t n_o,
                                                                      const uint64_t *__restrict__ bmask, const BrJob *__restrict__ jobs) {
    const BrJob j = jobs[blockIdx.z];
    br_terminal_boards_body<RAKED>(mask_p, score_p, pw, n_p, mask_o, score_o, j.q, n_o, bmask, j.uncontested, j.value, RAKED ? j.value_tie : 0.0, RAKED ? j.value_lose : 0.0,
                                   j.v);
}

// ---- the full-width sweep (rs_range_cfr_*): vector-form CFR over both ranges and every run-out on this walk, f32 tables ----------------------------------------------
// The opponent plays get_strategy of its regrets (the reach kernels above, handed the regret array), leaves and opponent nodes on the way up are the best response's.  New:
// the traverser's OWN reach pi goes down beside q (the strategy sums want it), and its own nodes keep the per-info-set sums RS_BR_MAX only compares:
//     S[a][c] = sum of vch[a][lane] over the info set's lanes, list order, from 0.0          U[c] = sum_a (double)sigma[a][c] * S[a][c], a ascending from 0.0
//     P[c]    = sum of pi[lane] over the same lanes in the same order
//     regret[a][c] = (float)((double)regret[a][c] + (S[a][c] - U[c]))   (RS_UPD_RMPLUS: a result that is not > 0.0f becomes 0.0f, visit_f32's rule)
//     ssum[a][c]   = (float)((double)ssum[a][c] + P[c] * (double)sigma[a][c])
//     v[lane]      = sum_a (double)sigma[a][c(lane)] * vch[a][lane], a ascending from 0.0       (RS_BR_AVERAGE's expression with the current strategy)
// sigma read from the regret row before it is written; every row written once per sweep.  Every addition has ONE order whatever form or tree order runs it.
// own node on the way down: pi_a[lane] = pi[lane] * sigma(cluster(lane), a).  (A lane that is no deal looks cluster 0 up, as the opponent's reach does: no list holds it.)
// The node report (rs_node_report) takes pi down the same way on every table type, handed the array its mode reads: get_strategy and get_final_strategy are one text.
template <int DT>
__device__ __forceinline__ void br_own_reach_lane(const void *__restrict__ regrets, BrNodeRow row, const uint32_t *__restrict__ cid, uint32_t h, uint32_t n_pad,
                                                  const double *__restrict__ pi, double *__restrict__ pi_out /*[A][n_pad]*/) {
    typename Elem<DT>::val r[RS_MAX_ACTIONS];
    float sig[RS_MAX_ACTIONS];
    current_sigma<DT>(regrets, row.cell_off, row.pitch, row.n_actions, cid[h], r, sig);
    const double ph = pi[h];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < row.n_actions) pi_out[(size_t)a * n_pad + h] = ph * (double)sig[a];
}
// sliced over the XCDs by hand as k_br_opp_reach_jobs: the regret rows are gathered by cluster id just as the strategy sums are there
template <int DT>
__global__ __launch_bounds__(kBrBlock) void k_br_own_reach_jobs(const void *__restrict__ regrets, const BrJob *__restrict__ jobs, uint32_t n, uint32_t n_pad, uint32_t n_hands) {
    const BrJob j = jobs[blockIdx.y];
    uint32_t h;
    if (!br_xcd_sliced_lane(n, n_hands, h)) return;
    br_own_reach_lane<DT>(regrets, j.row, j.cid, h, n_pad, j.q, j.q_out);
}

// the row writes of one info set: U from the sums, then regret and strategy-sum cells of every action
__device__ __forceinline__ void br_cfr_store(float *__restrict__ regrets, float *__restrict__ ssum, BrNodeRow row, uint32_t c, const float (&r)[RS_MAX_ACTIONS],
                                             const float (&sig)[RS_MAX_ACTIONS], const double (&s)[RS_MAX_ACTIONS], double P, int rmplus) {
    double U = 0.0;
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < row.n_actions) U += (double)sig[a] * s[a];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < row.n_actions) {
            const size_t at = row.cell_off + (size_t)a * row.pitch + c;
            float nr = (float)((double)r[a] + (s[a] - U));
            if (rmplus && !(nr > 0.0f)) nr = 0.0f;
            regrets[at] = nr;
            ssum[at] = (float)((double)ssum[at] + P * (double)sig[a]);
        }
}
// own node on the way up, one THREAD per info set: the list in steps of 8 lanes -- their ids once, then the pi and every (action, lane) value of the step in flight
// together (br_own_body's short-list trick; a river info set of a bucketed abstraction is one step), the additions in list order.  One pass: the step's lanes get their v
// while their values are in registers.
__device__ __forceinline__ void br_cfr_own_body(float *__restrict__ regrets, float *__restrict__ ssum, BrNodeRow row, const uint32_t *__restrict__ start /*[n_clusters + 2]*/,
                                                const uint32_t *__restrict__ order, uint32_t n_clusters, uint32_t n_pad, const double *__restrict__ vch,
                                                const double *__restrict__ pi, int rmplus, double *__restrict__ v) {
    for (uint32_t i = start[n_clusters] + blockIdx.x * kBrBlock + threadIdx.x; i < start[n_clusters + 1]; i += gridDim.x * kBrBlock) v[order[i]] = 0.0;   // no deal: worth 0
    const uint32_t c = blockIdx.x * kBrBlock + threadIdx.x;
    if (c >= n_clusters) return;
    const uint32_t lo = start[c], hi = start[c + 1];
    if (lo == hi) return;   // no dealt lane: the cells stay
    float r[RS_MAX_ACTIONS], sig[RS_MAX_ACTIONS];
    current_sigma<kDT_F32>(regrets, row.cell_off, row.pitch, row.n_actions, c, r, sig);
    double s[RS_MAX_ACTIONS];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++) s[a] = 0.0;
    double P = 0.0;
    for (uint32_t i = lo; i < hi; i += 8) {
        uint32_t idx[8];
        double tp[8], va[8];
#pragma unroll
        for (int k = 0; k < 8; k++) idx[k] = i + k < hi ? order[i + k] : order[lo];
#pragma unroll
        for (int k = 0; k < 8; k++) tp[k] = pi[idx[k]], va[k] = 0.0;
#pragma unroll
        for (int a = 0; a < RS_MAX_ACTIONS; a++)
            if ((uint32_t)a < row.n_actions) {
                const double *ra = vch + (size_t)a * n_pad;
                double t[8];
#pragma unroll
                for (int k = 0; k < 8; k++) t[k] = ra[idx[k]];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (i + k < hi) {
                        s[a] += t[k];
                        va[k] += (double)sig[a] * t[k];
                    }
            }
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (i + k < hi) {
                P += tp[k];
                v[idx[k]] = va[k];
            }
    }
    br_cfr_store(regrets, ssum, row, c, r, sig, s, P, rmplus);
}
// ... one WAVE per info set, where info sets hold many lanes (br_wave_per_info_set): 64 gathers per step and row, the additions one after the other in list order out of
// the neighbours' registers (br_own_wave_body), so every lane holds the thread form's sums, bit for bit; lane 0 writes the rows
__device__ __forceinline__ void br_cfr_own_wave_body(float *__restrict__ regrets, float *__restrict__ ssum, BrNodeRow row, const uint32_t *__restrict__ start,
                                                     const uint32_t *__restrict__ order, uint32_t n_clusters, uint32_t n_pad, const double *__restrict__ vch,
                                                     const double *__restrict__ pi, int rmplus, double *__restrict__ v) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * kBrBlock + threadIdx.x) >> 6, n_waves = gridDim.x * (kBrBlock >> 6);
    for (uint32_t i = start[n_clusters] + blockIdx.x * kBrBlock + threadIdx.x; i < start[n_clusters + 1]; i += gridDim.x * kBrBlock) v[order[i]] = 0.0;
    for (uint32_t c = wave; c < n_clusters; c += n_waves) {
        const uint32_t lo = start[c], hi = start[c + 1];
        if (lo == hi) continue;
        float r[RS_MAX_ACTIONS], sig[RS_MAX_ACTIONS];
        current_sigma<kDT_F32>(regrets, row.cell_off, row.pitch, row.n_actions, c, r, sig);
        double s[RS_MAX_ACTIONS];
#pragma unroll
        for (int a = 0; a < RS_MAX_ACTIONS; a++) s[a] = 0.0;
        double P = 0.0;
        for (uint32_t i = lo; i < hi; i += 64) {
            const uint32_t cnt = min(64u, hi - i);   // wave-uniform
            const uint32_t h = order[lane < cnt ? i + lane : lo];
            const double tp = lane < cnt ? pi[h] : 0.0;
            double va = 0.0;
#pragma unroll
            for (int a = 0; a < RS_MAX_ACTIONS; a++)
                if ((uint32_t)a < row.n_actions) {
                    const double t = lane < cnt ? vch[(size_t)a * n_pad + h] : 0.0;
                    va += (double)sig[a] * t;
                    const int t_lo = __double2loint(t), t_hi = __double2hiint(t);
                    double acc = s[a];
                    for (uint32_t k = 0; k < cnt; ++k) acc += __hiloint2double(__builtin_amdgcn_readlane(t_hi, (int)k), __builtin_amdgcn_readlane(t_lo, (int)k));
                    s[a] = acc;
                }
            const int p_lo = __double2loint(tp), p_hi = __double2hiint(tp);
            for (uint32_t k = 0; k < cnt; ++k) P += __hiloint2double(__builtin_amdgcn_readlane(p_hi, (int)k), __builtin_amdgcn_readlane(p_lo, (int)k));
            if (lane < cnt) v[h] = va;
        }
        if (lane == 0) br_cfr_store(regrets, ssum, row, c, r, sig, s, P, rmplus);
    }
}
__global__ __launch_bounds__(kBrBlock) void k_br_cfr_own_jobs(float *__restrict__ regrets, float *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n_pad, int rmplus) {
    const BrJob j = jobs[blockIdx.y];
    br_cfr_own_body(regrets, ssum, j.row, j.start, j.order, j.n_clusters, n_pad, j.vch, j.q, rmplus, j.v);
}
__global__ __launch_bounds__(kBrBlock) void k_br_cfr_own_wave_jobs(float *__restrict__ regrets, float *__restrict__ ssum, const BrJob *__restrict__ jobs, uint32_t n_pad,
                                                                   int rmplus) {
    const BrJob j = jobs[blockIdx.y];
    br_cfr_own_wave_body(regrets, ssum, j.row, j.start, j.order, j.n_clusters, n_pad, j.vch, j.q, rmplus, j.v);
}

// ---- the node report (rs_node_report): per (prefix of the node's round, hand) what RS_BR_AVERAGE's walk holds at a requested node ------------------------------------
// k_br_own_real_cols_jobs / _last_jobs' fold with the sums kept instead of compared: A + 2 lane rows -- the children's values vch[a], the node's own value row, the mass row (an
// uncontested leaf of value 1.0 on the node's q: the kBrMass job before this one) -- are added up over the run-outs of the pair's prefix, ascending from 0.0, lanes that are
// no deal not added; the last row is the traverser's own reach pi on the pair's first deal.  out: [A + 3][n_pairs], rows cfv[0 .. A), v, mass, own.
// Under RS_BR_AVERAGE no own node folds its opponent children (BrPlan's `folds`), so every child row and the node's own row stand written when the report runs: plain rows.
// A workgroup takes 64 neighbouring pairs (neighbouring threads neighbouring hands) and its four waves share the ROWS: each row's additions stay sequential down the
// run-outs, eight loads in flight.  Nothing is indexed by the action: a row is a pointer picked under a predicate, the sums never meet.
__device__ __forceinline__ const double *br_report_row(uint32_t row, uint32_t n_actions, uint32_t n_pad, const double *__restrict__ vch, const double *__restrict__ v,
                                                       const double *__restrict__ mass) {
    return row < n_actions ? vch + (size_t)row * n_pad : (row == n_actions ? v : mass);
}
__device__ __forceinline__ void br_report_cols_body(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n_pairs, uint32_t pp,
                                                    uint32_t n_pad, uint32_t n_actions, const double *__restrict__ vch, const double *__restrict__ v,
                                                    const double *__restrict__ mass, const double *__restrict__ pi, double *__restrict__ out) {
    const uint32_t x = threadIdx.x & 63u, w = threadIdx.x >> 6, pair = blockIdx.x * kBrRealPairs + x;
    if (pair >= n_pairs) return;
    const uint32_t f = pair / n_hands, h = pair - f * n_hands;
    const uint64_t mine = mask_p[h];
    const uint64_t *__restrict__ bm = bmask + (size_t)f * pp;
    const uint32_t lane0 = f * pp * n_hands + h;   // run-out k of the pair: lane0 + k * n_hands (below n < 2^31)
    for (uint32_t row = w; row < n_actions + 3; row += kBrRealWaves) {
        if (row == n_actions + 2) {   // own: pi is constant over the deals of a prefix, the lowest run-out speaks; 0.0 where the pair is no deal at all
            double own = 0.0;
            for (uint32_t k = 0; k < pp; k++)
                if (!(mine & bm[k])) {
                    own = pi[lane0 + k * n_hands];
                    break;
                }
            out[(size_t)row * n_pairs + pair] = own;
            continue;
        }
        const double *__restrict__ src = br_report_row(row, n_actions, n_pad, vch, v, mass);
        double acc = 0.0;
        for (uint32_t k = 0; k < pp; k += kBrRealFlight) {
            bool deal[kBrRealFlight];
            double t[kBrRealFlight];
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++) {
                const uint32_t kk = min(k + q, pp - 1);
                deal[q] = k + q < pp && !(mine & bm[kk]);
                t[q] = src[lane0 + kk * n_hands];
            }
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++)
                if (deal[q]) acc += t[q];   // ascending run-outs, one after the other
        }
        out[(size_t)row * n_pairs + pair] = acc;
    }
}
// the last round (one run-out per prefix): a pair is a lane, the fold one addition to 0.0 -- element-wise, every row read once and written once
__device__ __forceinline__ void br_report_last_body(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n, uint32_t n_pad,
                                                    uint32_t n_actions, const double *__restrict__ vch, const double *__restrict__ v, const double *__restrict__ mass,
                                                    const double *__restrict__ pi, double *__restrict__ out) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    const uint32_t b = lane / n_hands, h = lane - b * n_hands;
    const bool deal = !(mask_p[h] & bmask[b]);
    double t[RS_MAX_ACTIONS + 3];
#pragma unroll
    for (int row = 0; row < RS_MAX_ACTIONS + 2; row++)   // every row's value on its way before the first store
        t[row] = (uint32_t)row < n_actions + 2 ? br_report_row((uint32_t)row, n_actions, n_pad, vch, v, mass)[lane] : 0.0;
    const double own = pi[lane];
#pragma unroll
    for (int row = 0; row < RS_MAX_ACTIONS + 2; row++)
        if ((uint32_t)row < n_actions + 2) out[(size_t)row * n + lane] = deal ? 0.0 + t[row] : 0.0;
    out[(size_t)(n_actions + 2) * n + lane] = deal ? own : 0.0;
}
__global__ __launch_bounds__(kBrBlock) void k_br_report_cols_jobs(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n_pairs,
                                                                  uint32_t pp, uint32_t n_pad, const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_report_cols_body(mask_p, bmask, n_hands, n_pairs, pp, n_pad, jp->n_children, jp->vch, jp->v, jp->sum_src[0], jp->q, jp->q_out);
}
__global__ __launch_bounds__(kBrBlock) void k_br_report_last_jobs(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n,
                                                                  uint32_t n_pad, const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_report_last_body(mask_p, bmask, n_hands, n, n_pad, jp->n_children, jp->vch, jp->v, jp->sum_src[0], jp->q, jp->q_out);
}

// ---- the re-solving gadget (rs_range_cfr_set_gadget): a two-action node of the OPPONENT above the tree's root, one info set per opponent hand ------------------------
// Action 0 TERMINATE pays the hand alt[h] times the root's mass row, action 1 FOLLOW enters the tree.  Its rows regret[2][n] / ssum[2][n] (f32) live with the solver
// object.  Two actions, unrolled: nothing is indexed by an action, r0 / r1 and s0 / s1 are registers.
// get_strategy (infoset.rs:83-102) of one hand's gadget row, in registers
__device__ __forceinline__ void br_gadget_sigma(const float *__restrict__ regret, uint32_t n, uint32_t h, float &r0, float &r1, float &s0, float &s1) {
    r0 = regret[h];
    r1 = regret[(size_t)n + h];
    float norm = 0.0f;
    if (r0 > 0.0f) norm += r0;
    if (r1 > 0.0f) norm += r1;
    s0 = (norm > 0.0f) ? ((r0 > 0.0f) ? r0 / norm : 0.0f) : 0.5f;
    s1 = (norm > 0.0f) ? ((r1 > 0.0f) ? r1 / norm : 0.0f) : 0.5f;
}
// the resolver's sweep, on the way down: the opponent's reach at the tree's root is init_q * sigma[FOLLOW], the TERMINATE leaf's reach (init_q * sigma[TERMINATE]) * alt
__global__ __launch_bounds__(kBrBlock) void k_br_gadget_reach(const float *__restrict__ regret, const double *__restrict__ alt, uint32_t n_hands, uint32_t n,
                                                              const double *__restrict__ init_q, double *__restrict__ q_follow, double *__restrict__ q_term) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    const uint32_t h = lane % n_hands;
    float r0, r1, s0, s1;
    br_gadget_sigma(regret, n_hands, h, r0, r1, s0, s1);
    const double q = init_q[lane];
    q_follow[lane] = q * (double)s1;
    q_term[lane] = (q * (double)s0) * alt[h];
}
// the opponent's sweep, behind the root's value job: one THREAD per hand folds the root row vF (FOLLOW) and alt * mass (TERMINATE) over the run-outs, ascending from 0.0,
// lanes that are no deal not added (br_report_cols_body's test), kBrRealFlight loads of each row in flight; sigma is known before the fold, so the lanes get their v while
// their values are in registers; then the hand's four cells.  The last round (NB = 1) is the same lane text once: element-wise, as k_br_report_last_jobs is.
// (A thread per hand rather than k_br_report_cols_jobs' workgroup of 64 hands with waves sharing rows: there are two rows, not A + 2, their sums meet in U, and the kernel runs
// once per sweep over at most 1 326 hands -- neighbouring threads read neighbouring hands of a run-out either way.)
__global__ __launch_bounds__(kBrBlock) void k_br_gadget_own(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t NB,
                                                            float *__restrict__ regret, float *__restrict__ ssum, const double *__restrict__ alt,
                                                            const double *__restrict__ mass, double *v, int rmplus) {
    const uint32_t h = blockIdx.x * kBrBlock + threadIdx.x;
    if (h >= n_hands) return;
    const uint64_t mine = mask_p[h];
    const double al = alt[h];
    float r0, r1, s0, s1;
    br_gadget_sigma(regret, n_hands, h, r0, r1, s0, s1);
    double S0 = 0.0, S1 = 0.0, P = 0.0;
    bool any = false;
    auto take = [&](size_t lane, bool deal, double f, double m) {   // one lane of the hand, its two values in registers
        if (!deal) {
            v[lane] = 0.0;
            return;
        }
        const double vt = al * m;
        S0 += vt;   // ascending run-outs, one after the other
        S1 += f;
        P += 1.0;   // the opponent's own reach at the gadget is 1.0 on every lane
        any = true;
        double acc = 0.0;
        acc += (double)s0 * vt;
        acc += (double)s1 * f;
        v[lane] = acc;
    };
    if (NB == 1) {   // the last round: element-wise, each row read once and written once
        take(h, !(mine & bmask[0]), v[h], mass[h]);
    } else {
        for (uint32_t k = 0; k < NB; k += kBrRealFlight) {
            bool in[kBrRealFlight], deal[kBrRealFlight];
            double tf[kBrRealFlight], tm[kBrRealFlight];
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++) {
                const uint32_t kk = min(k + q, NB - 1);
                in[q] = k + q < NB;
                deal[q] = in[q] && !(mine & bmask[kk]);
                tf[q] = v[(size_t)kk * n_hands + h];
                tm[q] = mass[(size_t)kk * n_hands + h];
            }
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++)
                if (in[q]) take((size_t)(k + q) * n_hands + h, deal[q], tf[q], tm[q]);
        }
    }
    if (!any) return;   // no dealt lane: the cells stay
    double U = 0.0;
    U += (double)s0 * S0;
    U += (double)s1 * S1;
    float n0 = (float)((double)r0 + (S0 - U)), n1 = (float)((double)r1 + (S1 - U));
    if (rmplus && !(n0 > 0.0f)) n0 = 0.0f;
    if (rmplus && !(n1 > 0.0f)) n1 = 0.0f;
    regret[h] = n0;
    regret[(size_t)n_hands + h] = n1;
    ssum[h] = (float)((double)ssum[h] + P * (double)s0);
    ssum[(size_t)n_hands + h] = (float)((double)ssum[(size_t)n_hands + h] + P * (double)s1);
}
// a Discounted CFR tick on the gadget rows: rs_discount_dcfr's three factors, one f32 multiply per cell
__global__ __launch_bounds__(kBrBlock) void k_br_gadget_discount(float *__restrict__ regret, float *__restrict__ ssum, uint32_t cells, float d_pos, float d_neg, float d_sum) {
    const uint32_t i = blockIdx.x * kBrBlock + threadIdx.x;
    if (i >= cells) return;
    const float r = regret[i];
    regret[i] = r * (r > 0.0f ? d_pos : d_neg);
    ssum[i] = ssum[i] * d_sum;
}

// ---- per-hand root values (rs_best_response_hands) and the max-margin gadget (rs_range_cfr_set_gadget_kind, RS_GADGET_MAXMARGIN) ------------------------------------
// k_br_gadget_own's fold without its update: one THREAD per hand adds the root's value row and the root's mass row up over the run-outs, ascending from 0.0, lanes that
// are no deal not added, kBrRealFlight loads of each row in flight.  The last round (NB = 1) is the same text with a fold of one addition.  A hand without a dealt lane
// gets 0.0 twice.  Nothing is written but the two sums.  mass == nullptr (the max-margin gadget's sweeps: M is known): the value row alone, out_m is not written.
__global__ __launch_bounds__(kBrBlock) void k_br_hands_fold(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t NB,
                                                            const double *__restrict__ v, const double *__restrict__ mass, double *__restrict__ out_v,
                                                            double *__restrict__ out_m) {
    const uint32_t h = blockIdx.x * kBrBlock + threadIdx.x;
    if (h >= n_hands) return;
    const uint64_t mine = mask_p[h];
    double F = 0.0, M = 0.0;
    if (NB == 1) {
        const double tf = v[h], tm = mass ? mass[h] : 0.0;
        if (!(mine & bmask[0])) {
            F += tf;
            M += tm;
        }
    } else {
        for (uint32_t k = 0; k < NB; k += kBrRealFlight) {
            bool deal[kBrRealFlight];
            double tf[kBrRealFlight], tm[kBrRealFlight];
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++) {
                const uint32_t kk = min(k + q, NB - 1);
                deal[q] = k + q < NB && !(mine & bmask[kk]);
                tf[q] = v[(size_t)kk * n_hands + h];
                tm[q] = mass ? mass[(size_t)kk * n_hands + h] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kBrRealFlight; q++)
                if (deal[q]) {   // ascending run-outs, one after the other
                    F += tf[q];
                    M += tm[q];
                }
        }
    }
    out_v[h] = F;
    if (mass) out_m[h] = M;
}

// The max-margin gadget's sums over HANDS equal the ascending sequential f64 sum bit for bit: ONE workgroup stages the terms in LDS (1 326 hands at most, padded with
// +0.0 to a multiple of eight: a sum that starts at +0.0 never holds -0.0, so adding +0.0 changes no bit) and its thread 0 adds them in order, eight LDS loads on their
// way before the first addition.  Hands go to threads in trips of kBrBlock.
constexpr int kBrHandsMax = 1328;   // 1 326 two-card hands, padded to a multiple of eight
__device__ __forceinline__ double br_ordered_sum(const double *lds, uint32_t n8) {   // thread 0 only; n8 a multiple of eight
    double acc = 0.0;
    for (uint32_t i = 0; i < n8; i += 8) {
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = lds[i + q];
#pragma unroll
        for (int q = 0; q < 8; q++) acc += t[q];
    }
    return acc;
}
// rho of the hand-choice row (row 0) as it stands, in f64: regret matching over the LIVE hands (M[h] > 0: a hand without a dealt lane has M = 0.0).  Every thread of the
// workgroup calls it; term[] and sc[] are LDS.  Returns norm and the number of live hands through sc[0], sc[1].
__device__ __forceinline__ void br_mm_norm(const float *__restrict__ regret, const double *__restrict__ M, uint32_t n, uint32_t n8, double *term, double *sc) {
    for (uint32_t h = threadIdx.x; h < n8; h += kBrBlock) {
        double pos = 0.0;
        if (h < n) {
            const float r = regret[h];
            pos = (M[h] > 0.0 && r > 0.0f) ? (double)r : 0.0;
        }
        term[h] = pos;
    }
    __syncthreads();
    if (threadIdx.x == 0) sc[0] = br_ordered_sum(term, n8);
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < n8; h += kBrBlock) term[h] = (h < n && M[h] > 0.0) ? 1.0 : 0.0;   // the live hands, counted the same way (exact: small integers)
    __syncthreads();
    if (threadIdx.x == 0) sc[1] = br_ordered_sum(term, n8);
    __syncthreads();
}
__device__ __forceinline__ double br_mm_rho(float r, double M, double norm, double L) {
    if (!(M > 0.0)) return 0.0;
    if (norm > 0.0) return r > 0.0f ? (double)r / norm : 0.0;
    return 1.0 / L;
}
// the resolver's sweep, first launch: scale[h] = rho[h] / M[h] (0.0 for a dead hand) and out[1] = the sum of rho[h] * alt[h] over the live hands, ascending from 0.0
__global__ __launch_bounds__(kBrBlock) void k_br_mm_scale(const float *__restrict__ regret, const double *__restrict__ M, const double *__restrict__ alt, uint32_t n,
                                                          double *__restrict__ scale, double *__restrict__ out) {
    __shared__ double term[kBrHandsMax];
    __shared__ double sc[2];
    const uint32_t n8 = (n + 7u) & ~7u;
    br_mm_norm(regret, M, n, n8, term, sc);
    const double norm = sc[0], L = sc[1];
    for (uint32_t h = threadIdx.x; h < n8; h += kBrBlock) {
        double ta = 0.0;
        if (h < n) {
            const double m = M[h], rho = br_mm_rho(regret[h], m, norm, L);
            scale[h] = m > 0.0 ? rho / m : 0.0;
            if (m > 0.0) ta = rho * alt[h];
        }
        term[h] = ta;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[1] = br_ordered_sum(term, n8);
}
// ... second launch, as k_br_gadget_reach does: the opponent enters the tree with q[lane] = init_q[lane] * scale[h]
__global__ __launch_bounds__(kBrBlock) void k_br_mm_reach(const double *__restrict__ scale, uint32_t n_hands, uint32_t n, const double *__restrict__ init_q,
                                                          double *__restrict__ q_follow) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    q_follow[lane] = init_q[lane] * scale[lane % n_hands];
}
// the opponent's sweep, behind k_br_hands_fold (F, M): u[h] = F[h] / M[h] - alt[h], U = the sum of rho[h] * u[h] over the live hands, the hand-choice row's cells and the
// margins.  Dead hands keep their cells and get margin NaN.  Row 1 of the gadget's rows is neither read nor written.  out[0] = U.
__global__ __launch_bounds__(kBrBlock) void k_br_mm_update(float *__restrict__ regret, float *__restrict__ ssum, const double *__restrict__ F, const double *__restrict__ M,
                                                           const double *__restrict__ alt, uint32_t n, double *__restrict__ margin, double *__restrict__ out, int rmplus) {
    __shared__ double term[kBrHandsMax];
    __shared__ double sc[3];
    const uint32_t n8 = (n + 7u) & ~7u;
    br_mm_norm(regret, M, n, n8, term, sc);
    const double norm = sc[0], L = sc[1];
    for (uint32_t h = threadIdx.x; h < n8; h += kBrBlock) {
        double tu = 0.0;
        if (h < n) {
            const double m = M[h];
            if (m > 0.0) tu = br_mm_rho(regret[h], m, norm, L) * (F[h] / m - alt[h]);
        }
        term[h] = tu;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double U = br_ordered_sum(term, n8);
        sc[2] = U;
        out[0] = U;
    }
    __syncthreads();
    const double U = sc[2];
    for (uint32_t h = threadIdx.x; h < n; h += kBrBlock) {
        const double m = M[h];
        if (!(m > 0.0)) {
            margin[h] = __longlong_as_double(0x7ff8000000000000ll);
            continue;
        }
        const float r = regret[h];
        const double rho = br_mm_rho(r, m, norm, L), fm = F[h] / m, al = alt[h], u = fm - al;
        float nr = (float)((double)r + (u - U));
        if (rmplus && !(nr > 0.0f)) nr = 0.0f;
        regret[h] = nr;
        ssum[h] = (float)((double)ssum[h] + rho);
        margin[h] = al - fm;
    }
}

// ---- node locks (rs_node_locks): an action node whose acting player plays a given per-hand strategy, lock[(a * n_prefix + f) * n_hands + h] -------------------------
// Two element-wise kernels in plain lane order, a thread per lane = b * n_hands + h: the reach that comes in, the A lock values of the lane's (prefix, hand) pair
// (f = b / pp, pp the run-outs under a prefix of the node's round) and the A rows of q_out / vch are unit-stride 8-byte accesses.  Nothing is gathered by cluster id, so
// no XCD slicing.  An early-round node's lock (A * n_prefix * n_hands doubles) stays in cache; a last-round node's rows are as long as a lane row.  Everything indexed
// by the action is unrolled to RS_MAX_ACTIONS under the action count as a predicate (current_sigma's reason: indexed by a run-time count it becomes scratch).
// reach, either side: out[a][lane] = in[lane] * lock[a][f][h].  The opponent's q at its locked node and the traverser's own pi at its own (full-width sweep, node report).
// A lane that is no deal takes whatever the lock holds there, as k_br_opp_reach_jobs takes cluster 0's strategy: its reach is never looked at.
__device__ __forceinline__ void br_lock_reach_body(const double *__restrict__ lock, uint32_t pp, uint32_t n_hands, uint32_t n, uint32_t n_pad, uint32_t n_actions,
                                                   const double *__restrict__ in, double *__restrict__ out /*[A][n_pad]*/) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    const uint32_t b = lane / n_hands, h = lane - b * n_hands;
    const size_t n_pairs = (size_t)(n / n_hands / pp) * n_hands, pair = (size_t)(b / pp) * n_hands + h;
    const double x = in[lane];
    double s[RS_MAX_ACTIONS];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++) s[a] = (uint32_t)a < n_actions ? lock[(size_t)a * n_pairs + pair] : 0.0;   // every lock value on its way before the first store
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < n_actions) out[(size_t)a * n_pad + lane] = x * s[a];
}
// the traverser's locked node on the way up: v[lane] = sum_a lock[a][f][h] * vch[a][lane], a ascending from 0.0; 0.0 where the lane is no deal (what k_br_own* and
// k_br_cfr_own* leave there).  Nothing is maximised and no table row is touched.
__device__ __forceinline__ void br_lock_value_body(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, const double *__restrict__ lock, uint32_t pp,
                                                   uint32_t n_hands, uint32_t n, uint32_t n_pad, uint32_t n_actions, const double *__restrict__ vch,
                                                   double *__restrict__ v) {
    const uint32_t lane = blockIdx.x * kBrBlock + threadIdx.x;
    if (lane >= n) return;
    const uint32_t b = lane / n_hands, h = lane - b * n_hands;
    if (mask_p[h] & bmask[b]) {
        v[lane] = 0.0;
        return;
    }
    const size_t n_pairs = (size_t)(n / n_hands / pp) * n_hands, pair = (size_t)(b / pp) * n_hands + h;
    double s[RS_MAX_ACTIONS], t[RS_MAX_ACTIONS];
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++) {   // every value on its way before the first addition
        s[a] = (uint32_t)a < n_actions ? lock[(size_t)a * n_pairs + pair] : 0.0;
        t[a] = (uint32_t)a < n_actions ? vch[(size_t)a * n_pad + lane] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < RS_MAX_ACTIONS; a++)
        if ((uint32_t)a < n_actions) acc += s[a] * t[a];
    v[lane] = acc;
}
// a lock job (kBrLockReach, kBrLockValue): sum_src[0] = the lock's rows on the device, n_clusters = pp, n_children = A; a reach job carries its side's shape with it (one
// launch takes the opponent's q jobs and the traverser's pi jobs of a depth): n_sets = n_hands, kmax = the side's lanes, row.pitch = its n_pad
__global__ __launch_bounds__(kBrBlock) void k_br_lock_reach_jobs(const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_lock_reach_body(jp->sum_src[0], jp->n_clusters, jp->n_sets, jp->kmax, jp->row.pitch, jp->n_children, jp->q, jp->q_out);
}
__global__ __launch_bounds__(kBrBlock) void k_br_lock_value_jobs(const uint64_t *__restrict__ mask_p, const uint64_t *__restrict__ bmask, uint32_t n_hands, uint32_t n,
                                                                 uint32_t n_pad, const BrJob *__restrict__ jobs) {
    const BrJob *__restrict__ jp = jobs + blockIdx.y;
    br_lock_value_body(mask_p, bmask, jp->sum_src[0], jp->n_clusters, n_hands, n, n_pad, jp->n_children, jp->vch, jp->v);
}

}  // namespace rs
