// rs_ehs.hip -- exact expected hand strength against a random hand, and the EHS histograms of a whole flop or turn round: the front end of the abstraction
// generator (gen_abstraction/ehs.rs EHS::get_ehs, main.rs:58-70 get_bin, main.rs generate_histograms), with enumeration in place of the reference's Monte-Carlo
// calc_equity.  Semantics: include/rustsolver_amd.h.  Everything before the last division is an integer, so results depend on the cards alone.
//   * k_ehs: the lookup form, one hand per wave (7 cards) or per workgroup (5 / 6 cards), every opponent hand of every completion evaluated;
//   * k_ehs_round_hist: the sweep, one workgroup per board of the round.  The board's decode and its (hole pair, bin) counters over all run-outs, a uint16 histogram
//     in LDS (profiles/ehs.md), are sweep_board and board_histogram of rs_ehs_dev.hpp, shared with k_preflop_counts (rs_ochs.hip); what is the kernel's own is the
//     last step: normalise, hand_index, store.
// Cards and suits only ever select under predicates (no array indexed by a card): the kernels carry no scratch.  A byte that is no card never indexes LDS: lists are
// validated before use, and every card the kernels enumerate themselves comes out of a bit mask.
#include <cstring>
#include <string>

#include "rs_ehs_dev.hpp"

using namespace rs;

#define RS_HIP(call, what)                                   \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return rs::hip_fail(e_, what); \
    } while (0)

namespace rs {

constexpr int kEhsThreads = 256;         // the lookup form
constexpr int kEhsWaves = kEhsThreads / 64;

// ---- the lookup form ------------------------------------------------------------------------------------------------------------------------------------
// NC = 7: a wave per hand, the lanes share its 990 opponents.  NC = 5 / 6: a workgroup per hand, its waves share the 1081 / 46 completions.
template <int NC>
__global__ __launch_bounds__(kEhsThreads) void k_ehs(const uint8_t *__restrict__ cards, uint32_t n, uint32_t pitch, float *__restrict__ out, uint32_t *__restrict__ err) {
    constexpr uint32_t kPer = NC == 7 ? kEhsWaves : 1;                      // hands per workgroup and trip
    constexpr uint32_t kCompl = NC == 7 ? 1u : (NC == 6 ? 46u : kEhsPairs);  // completions of a hand
    __shared__ uint32_t acc[kEhsWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t base = blockIdx.x * kPer; base < n; base += gridDim.x * kPer) {
        if (threadIdx.x < kEhsWaves) acc[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t h = NC == 7 ? base + wave : base;
        const uint32_t slot = NC == 7 ? wave : 0;
        bool ok = h < n;
        uint64_t held = 0;
        uint32_t own[4] = {0, 0, 0, 0}, brd[4] = {0, 0, 0, 0};
        if (ok) {
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const uint32_t c = cards[(size_t)i * pitch + h];
                ok = ok && c < 52u;
                held |= 1ull << (c & 63u);
                if (i >= 2) add_card(brd, c);
                else add_card(own, c);
            }
            ok = ok && __popcll(held) == NC;
            if (!ok && (NC == 7 ? lane == 0 : threadIdx.x == 0)) atomicOr(err, 1u);
        }
        if (ok) {
            const uint64_t free0 = kDeck & ~held;   // 45 / 46 / 47 cards
            uint32_t sum = 0;                        // of 2 [opp < own] + [opp == own]
            for (uint32_t co = NC == 7 ? 0 : wave; co < kCompl; co += NC == 7 ? 1 : kEhsWaves) {
                uint32_t b[4] = {brd[0], brd[1], brd[2], brd[3]};
                uint64_t free7 = free0;
                if (NC == 6) {
                    const uint32_t c = nth_bit(free0, co);
                    add_card(b, c);
                    free7 &= ~(1ull << c);
                }
                if (NC == 5) {
                    uint32_t i, j;
                    pair_of<47>(co, i, j);
                    const uint32_t ci = nth_bit(free0, i), cj = nth_bit(free0, j);
                    add_card(b, ci);
                    add_card(b, cj);
                    free7 &= ~(1ull << ci | 1ull << cj);
                }
                const uint32_t mine[4] = {b[0] | own[0], b[1] | own[1], b[2] | own[2], b[3] | own[3]};
                const uint32_t s = evaluate_suits(mine);
                for (uint32_t o = lane; o < kEhsOpp; o += 64) {
                    uint32_t i, j;
                    pair_of<45>(o, i, j);
                    uint32_t m[4] = {b[0], b[1], b[2], b[3]};
                    add_card(m, nth_bit(free7, i));
                    add_card(m, nth_bit(free7, j));
                    const uint32_t so = evaluate_suits(m);
                    sum += so < s ? 2u : (so == s ? 1u : 0u);
                }
            }
            atomicAdd(&acc[slot], sum);
        }
        __syncthreads();
        if (ok && (NC == 7 ? lane == 0 : threadIdx.x == 0)) out[h] = (float)((double)acc[slot] / (double)(2u * kEhsOpp * kCompl));
        __syncthreads();
    }
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------------------------
struct EhsSweep {
    HandIndexView view;
    EhsBins bins;
    const uint8_t *boards;   // [nb][pitch], or nullptr: board number blockIdx.x of all C(52, nb)
    uint32_t pitch;
    int32_t nb;              // 3 or 4
    float *out;              // [size(1)][n_bins]
    uint32_t *err;
};

__global__ __launch_bounds__(kSweepThreads, 8) void k_ehs_round_hist(const EhsSweep a) {
    extern __shared__ uint32_t ehs_lds[];
    const HistLds l = carve_hist_lds(ehs_lds);
    const int nb = a.nb, n_bins = a.bins.n_bins;
    const uint32_t nf = 52u - (uint32_t)nb, n_hp = nf * (nf - 1) / 2;
    const uint32_t n_compl = nb == 3 ? kEhsPairs : 46u;   // run-outs of the board that take no card of a given hole pair: the completions of the hand
    const uint32_t tid = threadIdx.x;

    uint32_t bc[5], bm[4] = {0, 0, 0, 0};
    uint64_t board;
    if (!sweep_board(a.boards, a.pitch, nb, bc, board, bm)) {   // uniform over the workgroup: reported, nothing written
        if (tid == 0) atomicOr(a.err, 1u);
        return;
    }
    const uint64_t free0 = kDeck & ~board;   // nf cards
    board_histogram(nb, a.bins, free0, bm, l, tid);

    // normalise and scatter through the indexer; the card bytes of a hand stand in LDS (the sort buffer is free now) so that hand_index reads no private array
    uint8_t *hand = reinterpret_cast<uint8_t *>(l.sorted) + tid * 8u;
    for (uint32_t hp = tid; hp < n_hp; hp += kSweepThreads) {
        uint32_t lo, hi;
        pair_positions(hp, lo, hi);
        hand[0] = (uint8_t)nth_bit(free0, lo);
        hand[1] = (uint8_t)nth_bit(free0, hi);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nb) hand[2 + i] = (uint8_t)bc[i];
        const uint64_t row = hand_index(a.view, 1, hand);
        float *dst = a.out + row * (uint64_t)n_bins;
        for (int k = 0; k < n_bins; ++k) dst[k] = (float)hist_count(l.hist, hp * (uint32_t)n_bins + (uint32_t)k) / (float)n_compl;
    }
}

}  // namespace rs

extern "C" {

int rs_ehs_bin(float value, int n_bins) {
    if (n_bins < 1 || n_bins > RS_EHS_MAX_BINS) return fail(RS_ERR_INVALID, "rs_ehs_bin: n_bins must be 1..RS_EHS_MAX_BINS");
    float thr[RS_EHS_MAX_BINS];
    ehs_thresholds(n_bins, thr);
    for (int bin = n_bins - 1; bin > 0; --bin)
        if (value > thr[bin]) return bin;
    return 0;
}

int rs_ehs(rs_table *t, const uint8_t *d_cards, int n_cards, uint32_t n, float *d_out) {
    if (!t) return fail(RS_ERR_INVALID, "rs_ehs: NULL table");
    if (n_cards != 5 && n_cards != 6 && n_cards != 7) return fail(RS_ERR_INVALID, "rs_ehs: n_cards must be 5, 6 or 7 (two hole cards and a flop, turn or river board)");
    if (n && (!d_out || !d_cards)) return fail(RS_ERR_INVALID, "rs_ehs: NULL cards or output with n > 0");
    if (n == 0) return RS_OK;
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    const uint32_t pitch = uint32_t(round_up(n, kLanePad));
    const uint32_t per = n_cards == 7 ? uint32_t(kEhsWaves) : 1u;
    const dim3 grid(std::min((n + per - 1) / per, 65536u)), block(kEhsThreads);
    return launch_checked(t, "rs_ehs", "k_ehs", "a hand", [&](uint32_t *d_err) {
        if (n_cards == 7) hipLaunchKernelGGL(k_ehs<7>, grid, block, 0, t->stream, d_cards, n, pitch, d_out, d_err);
        else if (n_cards == 6) hipLaunchKernelGGL(k_ehs<6>, grid, block, 0, t->stream, d_cards, n, pitch, d_out, d_err);
        else hipLaunchKernelGGL(k_ehs<5>, grid, block, 0, t->stream, d_cards, n, pitch, d_out, d_err);
    });
}

int rs_ehs_round_histograms(rs_table *t, rs_hand_indexer *ix, int n_bins, const uint8_t *d_boards, uint32_t n_boards, float *d_out) {
    if (!t || !ix) return fail(RS_ERR_INVALID, "rs_ehs_round_histograms: NULL argument");
    const int nc = rs_hand_indexer_n_cards(ix, 1);
    if (rs_hand_indexer_rounds(ix) != 2 || rs_hand_indexer_n_cards(ix, 0) != 2 || (nc != 5 && nc != 6))
        return fail(RS_ERR_INVALID, "rs_ehs_round_histograms: the indexer must be hand_indexer_s::init(2, [2, 3]) (flop) or (2, [2, 4]) (turn)");
    if (n_bins < 1 || n_bins > RS_EHS_MAX_BINS) return fail(RS_ERR_INVALID, "rs_ehs_round_histograms: n_bins must be 1..RS_EHS_MAX_BINS");
    const int nb = nc - 2;
    if (!d_boards) n_boards = nb == 3 ? 22100u : 270725u;
    if (n_boards && !d_out) return fail(RS_ERR_INVALID, "rs_ehs_round_histograms: NULL output");
    if (n_boards == 0) return RS_OK;
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    EhsSweep a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = hand_indexer_view_on(ix, t->device, t->stream, &a.view)) return rc;
    ehs_thresholds(n_bins, a.bins.thr);
    a.bins.n_bins = n_bins;
    a.boards = d_boards;
    a.pitch = uint32_t(round_up(n_boards, kLanePad));
    a.nb = nb;
    a.out = d_out;
    const size_t lds = size_t(ehs_sweep_lds_words(nb, n_bins)) * sizeof(uint32_t);
    if (int rc = grant_lds(reinterpret_cast<const void *>(k_ehs_round_hist), lds, "rs_ehs_round_histograms")) return rc;
    return launch_checked(t, "rs_ehs_round_histograms", "k_ehs_round_hist", "a board", [&](uint32_t *d_err) {
        a.err = d_err;
        hipLaunchKernelGGL(k_ehs_round_hist, dim3(n_boards), dim3(kSweepThreads), lds, t->stream, a);
    });
}

}  // extern "C"
