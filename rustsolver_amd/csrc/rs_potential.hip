// rs_potential.hip -- potential-aware abstraction (Ganzfried and Sandholm, AAAI 2014): a flop or turn hand described by its distribution over the NEXT round's buckets,
// and a k-means over such rows under the paper's greedy earth mover's distance (Algorithm 2).  Semantics: include/rustsolver_amd.h; DESIGN.md section 4.
//   * k_next_round_rows: one workgroup per board, a wave per hole pair at a time, a lane per next card.  The hand's card bytes stand in LDS (as in k_ochs_round's last
//     step), the lane indexes the hand of the next round and reads its bucket; the wave sorts its 64 keys (idle lanes hold kNoKey) with shuffles and run-length encodes them
//     with a ballot and a prefix popcount.  The board's decode, the pair numbering, class_boards and launch_checked are rs_ehs_dev.hpp's and rs_ochs.hip's.
//   * k_pa_assign: a wave (one workgroup) per point, lanes = the point's entries (at most 47), which stay in registers over the loop of means.  The mean's row is copied
//     into LDS (`rem`); every lane keeps its own neighbour rank and runs ahead over buckets that are empty -- an empty bucket stays empty, so nothing is lost -- and the
//     wave only ever executes the takes of the LOWEST rank any live lane stands at: every take of a lower rank has happened, which is the (rank, entry) order of the
//     definition.  A lane looks through two 8-byte words of its row of `order` itself (four ranks and four LDS reads each); past that the whole wave looks for it,
//     64 ranks to a coalesced load and a ballot.  The lowest rank is found by ballots, bit by bit.  One lane alone at that rank takes at once; several take in
//     ascending entry order where they meet a bucket: an LDS atomicMin ticket per bucket (64 slots by the bucket's low bits; two buckets on one slot only cost a
//     round).  The walk ends when every entry is done or no lane finds a positive bucket.
//   * k_pa_sums / k_pa_means: the integer sums of the members' counts (uint32 atomicAdd: no order) and the one f64 division per cell.
// A workgroup of k_pa_assign is one wave, so its barriers order the wave's LDS traffic and cost no s_barrier.  No kernel here carries scratch (profiles/potential.md).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "rs_ehs_dev.hpp"

using namespace rs;

#define RS_HIP(call, what)                                   \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return rs::hip_fail(e_, what); \
    } while (0)

struct rs_pa_metric {
    int n_next = 0;
    uint32_t pitch = 0;             // ids per row of `order`: n_next rounded up to 4, so that a lane loads four ranks in one 8-byte word
    int device = -1;                // -1: host only
    std::vector<float> ground;      // [n_next][n_next]
    std::vector<uint16_t> order;    // [n_next][pitch]
    DevBuf<float> d_ground;
    DevBuf<uint16_t> d_order;
};

namespace rs {

constexpr uint32_t kRowWords = RS_PA_ROW_WORDS;
constexpr uint32_t kErrBoard = 1u, kErrBucket = 2u, kErrRow = 1u;

// ---- the rows ---------------------------------------------------------------------------------------------------------------------------------------------------
struct NextSweep {
    HandIndexView view, next;   // [2, nb] and [2, nb + 1]
    const uint8_t *boards;      // [nb][pitch]
    uint32_t pitch;
    int32_t nb;                 // 3 or 4
    uint32_t n_next;
    const uint32_t *buckets;    // [size(next, 1)]
    uint32_t *rows;             // [size(view, 1)][kRowWords]
    uint32_t *err;
};

constexpr int kNextThreads = 256;

__global__ __launch_bounds__(kNextThreads) void k_next_round_rows(const NextSweep a) {
    __shared__ uint8_t hands[kNextThreads * 8];
    const int nb = a.nb;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t bc[5], bm[4] = {0, 0, 0, 0};
    uint64_t board;
    __builtin_assume(a.boards != nullptr);   // the host always lists the boards (class_boards)
    if (!sweep_board(a.boards, a.pitch, nb, bc, board, bm)) {   // uniform over the workgroup: reported, nothing written
        if (tid == 0) atomicOr(a.err, kErrBoard);
        return;
    }
    const uint64_t free0 = kDeck & ~board;
    const uint32_t nf = 52u - (uint32_t)nb, n_hp = nf * (nf - 1) / 2, n_draws = nf - 2u;
    uint8_t *hand = hands + tid * 8u;   // this thread's own bytes: hole pair, board, next card
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < nb) hand[2 + i] = (uint8_t)bc[i];

    for (uint32_t hp = wave; hp < n_hp; hp += kNextThreads / 64) {
        uint32_t lo, hi;
        pair_positions(hp, lo, hi);
        const uint32_t c0 = nth_bit(free0, lo), c1 = nth_bit(free0, hi);
        const uint64_t free2 = free0 & ~(1ull << c0 | 1ull << c1);   // n_draws cards
        hand[0] = (uint8_t)c0;
        hand[1] = (uint8_t)c1;
        const uint64_t row = hand_index(a.view, 1, hand);
        uint32_t key = kNoKey;
        bool bad = false;
        if (lane < n_draws) {
            hand[2 + nb] = (uint8_t)nth_bit(free2, lane);
            key = a.buckets[hand_index(a.next, 1, hand)];
            bad = key >= a.n_next;
        }
        if (__ballot(bad)) {   // uniform over the wave: reported, the hand's row left as it was
            if (lane == 0) atomicOr(a.err, kErrBucket);
            continue;
        }
        // ascending bitonic sort of the wave's 64 keys
#pragma unroll
        for (uint32_t k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)key, (int)j);
                const bool keep_low = ((lane & j) == 0) == ((lane & k) == 0);
                key = keep_low ? (key < other ? key : other) : (key > other ? key : other);
            }
        // run-length encoding: a run's first lane writes `bucket << 8 | length` at the run's number
        const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
        const bool head = key != kNoKey && (lane == 0 || key != prev);
        const uint64_t heads = __ballot(head), bounds = __ballot(head || key == kNoKey);
        const uint32_t n_runs = (uint32_t)__popcll(heads);
        uint32_t *dst = a.rows + row * kRowWords;
        if (head) {
            const uint64_t rest = lane == 63u ? 0ull : bounds >> (lane + 1u);
            const uint32_t next = rest ? lane + 1u + (uint32_t)__builtin_ctzll(rest) : 64u;
            dst[__popcll(heads & ((1ull << lane) - 1ull))] = key << 8 | (next - lane);
        }
        if (lane >= n_runs && lane < kRowWords) dst[lane] = 0;
    }
}

// ---- the assignment -----------------------------------------------------------------------------------------------------------------------------------------------
struct PaAssign {
    const uint32_t *rows;      // [.][kRowWords]
    const uint32_t *sel;       // may be null
    size_t n;
    uint32_t n_draws, n_next, pitch;
    const float *means;        // [n_means][n_next]
    int32_t n_means;
    const uint16_t *order;     // [n_next][pitch]
    const float *ground;       // [n_next][n_next]
    uint32_t *clusters;        // may be null
    float *min_dist;           // may be null
    uint32_t *changed;         // may be null: counts the data whose cluster differs from clusters[i] as it stood
    uint32_t *err;
};

__host__ __device__ inline uint32_t pa_lds_words(uint32_t n_next) { return (n_next + 63u) / 64u * 64u + 64u; }   // rem, the tickets

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// the row's entries, one per lane: false unless the row is well-formed (include/rustsolver_amd.h).  m = its entries
__device__ __forceinline__ bool row_entries(uint32_t w, uint32_t lane, uint32_t n_next, uint32_t n_draws, uint32_t &m) {
    const uint64_t used = __ballot(w != 0);
    m = (uint32_t)__popcll(used);
    const uint32_t prev = (uint32_t)__shfl_up((int)w, 1);
    const bool wrong = w != 0 && ((w & 255u) == 0 || (w >> 8) >= n_next || (lane > 0 && (w >> 8) <= (prev >> 8)));
    return (used & (used + 1ull)) == 0 && m >= 1 && !__ballot(wrong) && (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_sum(w & 255u)) == n_draws;   // wave-uniform
}

__global__ __launch_bounds__(64) void k_pa_assign(const PaAssign a) {
    extern __shared__ uint32_t pa_lds[];
    float *rem = reinterpret_cast<float *>(pa_lds);                 // [n_next] what is left of the mean
    uint32_t *ticket = pa_lds + (pa_lds_words(a.n_next) - 64u);     // [64]
    const uint32_t lane = threadIdx.x, n_next = a.n_next;

    for (size_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const size_t r = a.sel ? a.sel[i] : i;
        const uint32_t w = lane < kRowWords ? a.rows[r * kRowWords + lane] : 0u;
        uint32_t m;
        if (!row_entries(w, lane, n_next, a.n_draws, m)) {   // uniform: reported, the datum's outputs left as they were
            if (lane == 0) atomicOr(a.err, kErrRow);
            continue;
        }
        const bool mine = w != 0;
        const uint32_t bkt = mine ? w >> 8 : 0u;
        const float target0 = (float)(w & 255u) / (float)a.n_draws;
        const uint64_t *ord = reinterpret_cast<const uint64_t *>(a.order + (size_t)bkt * a.pitch);   // four ranks to a word
        const float *gr = a.ground + (size_t)bkt * n_next;
        const uint32_t last_word = a.pitch / 4u - 1u;

        uint32_t best = 0;
        float best_v = 0.0f;
        for (int k = 0; k < a.n_means; ++k) {
            const float *q = a.means + (size_t)k * n_next;
            __syncthreads();   // the walk before has read its last
            for (uint32_t t = lane; t < n_next; t += 64u) rem[t] = q[t];
            __syncthreads();

            float target = target0, tot = 0.0f, d = 0.0f;
            uint32_t rk = mine ? 0u : n_next;   // this entry's neighbour rank; n_next: done, or nothing left to find
            uint32_t at = 0, d_of = 0xffffffffu;   // the word of `ord` in `ids` (the one after it waits in `ahead`); the bucket `d` was read for
            uint64_t ids = ord[0], ahead = ord[last_word ? 1u : 0u];
            auto take = [&](uint32_t t) {        // this entry's step at bucket t: the definition's two branches
                const float have = rem[t];
                ++rk;
                if (have > 0.0f) {               // else: an earlier entry emptied it at this rank
                    if (have < target) {
                        tot += have * d;
                        target -= have;
                        rem[t] = 0.0f;
                    } else {
                        tot += target * d;
                        rem[t] = have - target;
                        target = 0.0f;
                        rk = n_next;
                    }
                }
            };
            for (;;) {
                uint32_t t = 0;
                bool far = false;                // two words of ranks held nothing: the wave looks further for this lane
                for (int words = 0; rk < n_next; ++words) {   // ahead over the empty buckets, four ranks at a time
                    if (words == 2) {
                        far = true;
                        break;
                    }
                    const uint32_t word = rk >> 2;
                    if (word != at) {
                        ids = word == at + 1u ? ahead : ord[word];
                        at = word;
                        ahead = ord[word < last_word ? word + 1u : last_word];
                    }
                    const uint32_t i0 = (uint32_t)ids & 0xffffu, i1 = (uint32_t)(ids >> 16) & 0xffffu, i2 = (uint32_t)(ids >> 32) & 0xffffu, i3 = (uint32_t)(ids >> 48);
                    const float r0 = rem[i0], r1 = rem[i1], r2 = rem[i2], r3 = rem[i3];   // ids past n_next are padding (0): read, never used
                    const uint32_t base = word << 2;
                    uint32_t found = n_next;
                    if (base + 3u >= rk && base + 3u < n_next && r3 > 0.0f) found = base + 3u, t = i3;
                    if (base + 2u >= rk && base + 2u < n_next && r2 > 0.0f) found = base + 2u, t = i2;
                    if (base + 1u >= rk && base + 1u < n_next && r1 > 0.0f) found = base + 1u, t = i1;
                    if (base >= rk && r0 > 0.0f) found = base, t = i0;
                    if (found < n_next) {
                        rk = found;
                        break;
                    }
                    rk = base + 4u < n_next ? base + 4u : n_next;
                }
                // the long way, lane by lane with the whole wave: 64 ranks of the lane's row of `order` in one coalesced load, the first positive bucket by a ballot
                for (uint64_t need = __ballot(far); need; need &= need - 1ull) {
                    const int j = __builtin_ctzll(need);
                    const uint16_t *row = a.order + (size_t)(uint32_t)__builtin_amdgcn_readlane((int)bkt, j) * a.pitch;
                    uint32_t from = (uint32_t)__builtin_amdgcn_readlane((int)rk, j), found = n_next, found_t = 0;
                    for (; from < n_next; from += 64u) {
                        const uint32_t r = from + lane;
                        uint32_t id = 0;
                        bool positive = false;
                        if (r < n_next) {
                            id = row[r];
                            positive = rem[id] > 0.0f;
                        }
                        const uint64_t hits = __ballot(positive);
                        if (hits) {
                            const int first = __builtin_ctzll(hits);
                            found = from + (uint32_t)first;
                            found_t = (uint32_t)__builtin_amdgcn_readlane((int)id, first);
                            break;
                        }
                    }
                    if (lane == (uint32_t)j) {
                        rk = found;
                        t = found_t;
                    }
                }
                if (rk < n_next && t != d_of) {  // the ground distance of the step, asked for before the wave agrees on the rank
                    d = gr[t];
                    d_of = t;
                }
                // the lowest rank any live lane stands at, bit by bit from the top: `lowest` ends as the lanes that stand there
                uint64_t lowest = __ballot(rk < n_next);
                if (!lowest) break;
#pragma unroll
                for (int bit = 13; bit >= 0; --bit) {   // a rank is below RS_PA_MAX_NEXT = 2^13; bit 13 only separates n_next = 8192 itself
                    const uint64_t zero = lowest & ~__ballot((rk >> bit) & 1u);
                    if (zero) lowest = zero;
                }
                bool pending = (lowest >> lane) & 1ull;   // the takes of that rank, same buckets in ascending entry order
                if ((lowest & (lowest - 1ull)) == 0) {   // one lane alone: no ticket
                    if (pending) take(t);
                    __syncthreads();
                    continue;
                }
                while (__ballot(pending)) {
                    if (pending) ticket[t & 63u] = 0xffffffffu;
                    __syncthreads();
                    if (pending) atomicMin(&ticket[t & 63u], lane);
                    __syncthreads();
                    if (pending && ticket[t & 63u] == lane) {
                        pending = false;
                        take(t);
                    }
                    __syncthreads();
                }
            }
            float v = 0.0f;
            for (uint32_t j = 0; j < m; ++j) v += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tot), (int)j));
            if (k == 0 || v < best_v) {          // first mean, then strictly smaller only
                best_v = v;
                best = (uint32_t)k;
            }
        }
        if (lane == 0) {
            if (a.changed && a.clusters[i] != best) atomicAdd(a.changed, 1u);
            if (a.clusters) a.clusters[i] = best;
            if (a.min_dist) a.min_dist[i] = best_v;
        }
    }
}

// ---- the means ----------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int kSumThreads = 256;

// sums[k][b] += the counts of the members of k, members[k] += 1: a wave per datum; a datum in no cluster (a row that is not well-formed) adds nothing
__global__ __launch_bounds__(kSumThreads) void k_pa_sums(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ sel, size_t n, const uint32_t *__restrict__ clusters,
                                                         uint32_t n_means, uint32_t n_next, uint32_t *__restrict__ sums, uint32_t *__restrict__ members) {
    const uint32_t lane = threadIdx.x & 63u;
    for (size_t i = (size_t)blockIdx.x * (kSumThreads / 64) + (threadIdx.x >> 6); i < n; i += (size_t)gridDim.x * (kSumThreads / 64)) {
        const uint32_t k = clusters[i];
        if (k >= n_means) continue;
        const size_t r = sel ? sel[i] : i;
        const uint32_t w = lane < kRowWords ? rows[r * kRowWords + lane] : 0u;
        if (w != 0 && (w >> 8) < n_next) atomicAdd(&sums[(size_t)k * n_next + (w >> 8)], w & 255u);
        if (lane == 0) atomicAdd(&members[k], 1u);
    }
}

__global__ __launch_bounds__(kSumThreads) void k_pa_means(const uint32_t *__restrict__ sums, const uint32_t *__restrict__ members, size_t cells, uint32_t n_next,
                                                          uint32_t n_draws, float *__restrict__ means) {
    for (size_t c = (size_t)blockIdx.x * kSumThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kSumThreads) {
        const uint32_t mem = members[c / n_next];
        if (mem) means[c] = (float)((double)sums[c] / ((double)mem * (double)n_draws));   // a cluster without members keeps its mean
    }
}

}  // namespace rs

namespace {

// the greedy distance on the host, (rank, entry) lockstep as the header states it; `rem` is the caller's scratch of n_next floats
float pa_distance(const rs_pa_metric &mt, const uint32_t *row, int m, int n_draws, const float *mean, std::vector<float> &rem) {
    const int n = mt.n_next;
    rem.assign(mean, mean + n);
    float target[RS_PA_ROW_WORDS], tot[RS_PA_ROW_WORDS];
    bool done[RS_PA_ROW_WORDS];
    for (int j = 0; j < m; ++j) {
        target[j] = (float)(row[j] & 255u) / (float)n_draws;
        tot[j] = 0.0f;
        done[j] = false;
    }
    int open = m, positive = 0;
    for (int t = 0; t < n; ++t) positive += rem[size_t(t)] > 0.0f;
    for (int i = 0; i < n && open && positive; ++i)   // both exits leave the bits unchanged: nothing more can be taken
        for (int j = 0; j < m; ++j) {
            if (done[j]) continue;
            const uint32_t b = row[j] >> 8;
            const uint32_t t = mt.order[size_t(b) * mt.pitch + size_t(i)];
            const float a = rem[t];
            if (!(a > 0.0f)) continue;
            const float d = mt.ground[size_t(b) * size_t(n) + t];
            if (a < target[j]) {
                tot[j] += a * d;
                target[j] -= a;
                rem[t] = 0.0f;
                --positive;
            } else {
                tot[j] += target[j] * d;
                rem[t] = a - target[j];
                if (!(rem[t] > 0.0f)) --positive;
                target[j] = 0.0f;
                done[j] = true;
                --open;
            }
        }
    float dist = 0.0f;
    for (int j = 0; j < m; ++j) dist += tot[j];
    return dist;
}

// the entries of a well-formed row, or -1
int row_entries_host(const uint32_t *row, int n_next, int n_draws) {
    int m = 0, sum = 0;
    while (m < RS_PA_ROW_WORDS && row[m] != 0) ++m;
    for (int j = m; j < RS_PA_ROW_WORDS; ++j)
        if (row[j] != 0) return -1;
    for (int j = 0; j < m; ++j) {
        if ((row[j] & 255u) == 0 || (row[j] >> 8) >= (uint32_t)n_next || (j > 0 && (row[j] >> 8) <= (row[j - 1] >> 8))) return -1;
        sum += int(row[j] & 255u);
    }
    return m >= 1 && sum == n_draws ? m : -1;
}

bool plain_values(const float *x, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || x[i] < 0.0f) return false;
    return true;
}

int check_pa(const char *who, const rs_table *t, const rs_pa_metric *mt, const void *d_rows, size_t n, int n_draws, const float *means, int n_means) {
    if (!t || !mt || !means || (!d_rows && n)) return fail(RS_ERR_INVALID, std::string(who) + ": NULL argument");
    if (mt->device != t->device) return fail(RS_ERR_INVALID, std::string(who) + ": the metric was not created on this table's device (a host-only metric serves rs_pa_distance alone)");
    if (n_draws < 1 || n_draws > 47) return fail(RS_ERR_INVALID, std::string(who) + ": n_draws must be 1..47");
    if (n_means < 1) return fail(RS_ERR_INVALID, std::string(who) + ": no means");
    if (!plain_values(means, size_t(n_means) * size_t(mt->n_next))) return fail(RS_ERR_INVALID, std::string(who) + ": a mean value is negative or not finite");
    return RS_OK;
}

int launch_assign(rs_table *t, PaAssign &a, uint32_t *d_err) {
    const size_t lds = size_t(pa_lds_words(a.n_next)) * sizeof(uint32_t);
    if (int rc = grant_lds(reinterpret_cast<const void *>(k_pa_assign), lds, "rs_pa_predict")) return rc;
    a.err = d_err;
    hipLaunchKernelGGL(k_pa_assign, dim3((unsigned)std::min<size_t>(a.n, 1u << 16)), dim3(64), lds, t->stream, a);
    return RS_OK;
}

PaAssign assign_args(const rs_pa_metric *mt, const uint32_t *d_rows, const uint32_t *d_sel, size_t n, int n_draws, const float *d_means, int n_means) {
    PaAssign a;
    std::memset(&a, 0, sizeof(a));
    a.rows = d_rows;
    a.sel = d_sel;
    a.n = n;
    a.n_draws = uint32_t(n_draws);
    a.n_next = uint32_t(mt->n_next);
    a.pitch = mt->pitch;
    a.means = d_means;
    a.n_means = n_means;
    a.order = mt->d_order;
    a.ground = mt->d_ground;
    return a;
}

}  // namespace

extern "C" {

int rs_next_round_histograms(rs_table *t, rs_hand_indexer *ix, rs_hand_indexer *next, const uint32_t *d_next_buckets, int n_next, const uint8_t *d_boards,
                             uint32_t n_boards, uint32_t *d_rows) {
    if (!t || !ix || !next) return fail(RS_ERR_INVALID, "rs_next_round_histograms: NULL argument");
    const int nc = rs_hand_indexer_n_cards(ix, 1);
    if (rs_hand_indexer_rounds(ix) != 2 || rs_hand_indexer_n_cards(ix, 0) != 2 || (nc != 5 && nc != 6) || rs_hand_indexer_rounds(next) != 2 ||
        rs_hand_indexer_n_cards(next, 0) != 2 || rs_hand_indexer_n_cards(next, 1) != nc + 1)
        return fail(RS_ERR_INVALID, "rs_next_round_histograms: the indexers must be hand_indexer_s::init(2, [2, 3]) with (2, [2, 4]) (flop) or (2, [2, 4]) with (2, [2, 5]) (turn)");
    if (n_next < 1 || n_next > RS_PA_MAX_NEXT) return fail(RS_ERR_INVALID, "rs_next_round_histograms: n_next must be 1..RS_PA_MAX_NEXT");
    if ((!d_boards || n_boards) && (!d_rows || !d_next_buckets)) return fail(RS_ERR_INVALID, "rs_next_round_histograms: NULL buffer");
    if (d_boards && n_boards == 0) return RS_OK;
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    const int nb = nc - 2;
    NextSweep a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = hand_indexer_view_on(ix, t->device, t->stream, &a.view)) return rc;
    if (int rc = hand_indexer_view_on(next, t->device, t->stream, &a.next)) return rc;
    DevBuf<uint8_t> d_classes;   // the whole round: one board per suit-isomorphism class reaches every canonical row
    a.boards = d_boards;
    a.pitch = uint32_t(round_up(n_boards, kLanePad));
    if (!d_boards) {
        std::vector<uint8_t> rows;
        if (int rc = class_boards(nb, &rows, &n_boards, &a.pitch)) return rc;
        RS_HIP(d_classes.alloc(rows.size()), "rs_next_round_histograms: the round's boards");
        RS_HIP(hipMemcpyAsync(d_classes, rows.data(), rows.size(), hipMemcpyHostToDevice, t->stream), "rs_next_round_histograms");
        RS_HIP(hipStreamSynchronize(t->stream), "rs_next_round_histograms");   // `rows` leaves scope
        a.boards = d_classes;
    }
    a.nb = nb;
    a.n_next = uint32_t(n_next);
    a.buckets = d_next_buckets;
    a.rows = d_rows;
    uint32_t word = 0;
    if (int rc = launch_checked(t, "rs_next_round_histograms", "k_next_round_rows", "a board", [&](uint32_t *d_err) {
            a.err = d_err;
            hipLaunchKernelGGL(k_next_round_rows, dim3(n_boards), dim3(kNextThreads), 0, t->stream, a);
        }, &word))
        return rc;
    if (word & kErrBoard)
        return fail(RS_ERR_INVALID, "rs_next_round_histograms: a board repeats a card or holds a byte that is not a card (0..51); nothing was written for it");
    if (word & kErrBucket) return fail(RS_ERR_INVALID, "rs_next_round_histograms: a next-round bucket is not below n_next; nothing was written for the hands that reach it");
    return RS_OK;
}

int rs_pa_metric_create(rs_table *t, const float *ground, int n_next, rs_pa_metric **out) {
    if (!ground || !out) return fail(RS_ERR_INVALID, "rs_pa_metric_create: NULL argument");
    if (n_next < 1 || n_next > RS_PA_MAX_NEXT) return fail(RS_ERR_INVALID, "rs_pa_metric_create: n_next must be 1..RS_PA_MAX_NEXT");
    const size_t n = size_t(n_next);
    if (!plain_values(ground, n * n)) return fail(RS_ERR_INVALID, "rs_pa_metric_create: a ground distance is negative or not finite");
    if (t)
        if (int rc_ = rs::table_settle(t, false)) return rc_;   // the uploads below synchronise the device
    rs_pa_metric *m = new rs_pa_metric;
    m->n_next = n_next;
    m->pitch = uint32_t(round_up(n, 4));
    m->ground.assign(ground, ground + n * n);
    m->order.assign(n * m->pitch, 0);
    std::vector<uint16_t> ids(n);
    for (size_t b = 0; b < n; ++b) {
        std::iota(ids.begin(), ids.end(), uint16_t(0));
        const float *g = ground + b * n;
        std::stable_sort(ids.begin(), ids.end(), [g](uint16_t x, uint16_t y) { return g[x] < g[y]; });
        std::copy(ids.begin(), ids.end(), m->order.begin() + b * m->pitch);
    }
    if (t) {
        hipError_t e = hipSetDevice(t->device);
        if (e == hipSuccess) e = m->d_ground.alloc(n * n);
        if (e == hipSuccess) e = m->d_order.alloc(m->order.size());
        if (e == hipSuccess) e = hipMemcpy(m->d_ground, m->ground.data(), n * n * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(m->d_order, m->order.data(), m->order.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            delete m;
            return hip_fail(e, "rs_pa_metric_create: the metric's device copy");
        }
        m->device = t->device;
    }
    *out = m;
    return RS_OK;
}

void rs_pa_metric_destroy(rs_pa_metric *m) { delete m; }

int rs_pa_distance(const rs_pa_metric *mt, const uint32_t *row, int n_draws, const float *mean, float *out) {
    if (!mt || !row || !mean || !out) return fail(RS_ERR_INVALID, "rs_pa_distance: NULL argument");
    if (n_draws < 1 || n_draws > 47) return fail(RS_ERR_INVALID, "rs_pa_distance: n_draws must be 1..47");
    const int m = row_entries_host(row, mt->n_next, n_draws);
    if (m < 0)
        return fail(RS_ERR_INVALID, "rs_pa_distance: the row is not well-formed (entries `bucket << 8 | count`, count >= 1, buckets ascending and below n_next, counts summing to n_draws, then zeros)");
    if (!plain_values(mean, size_t(mt->n_next))) return fail(RS_ERR_INVALID, "rs_pa_distance: a mean value is negative or not finite");
    std::vector<float> rem;
    *out = pa_distance(*mt, row, m, n_draws, mean, rem);
    return RS_OK;
}

int rs_pa_predict(rs_table *t, const rs_pa_metric *mt, const uint32_t *d_rows, const uint32_t *d_sel, size_t n, int n_draws, const float *means, int n_means,
                  uint32_t *d_clusters, float *d_min_dist) {
    if (int rc = check_pa("rs_pa_predict", t, mt, d_rows, n, n_draws, means, n_means)) return rc;
    if (n == 0 || (!d_clusters && !d_min_dist)) return RS_OK;
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    const size_t cells = size_t(n_means) * size_t(mt->n_next);
    DevBuf<float> d_means;
    RS_HIP(d_means.alloc(cells), "rs_pa_predict: the means");
    RS_HIP(hipMemcpyAsync(d_means, means, cells * sizeof(float), hipMemcpyHostToDevice, t->stream), "rs_pa_predict");
    PaAssign a = assign_args(mt, d_rows, d_sel, n, n_draws, d_means, n_means);
    a.clusters = d_clusters;
    a.min_dist = d_min_dist;
    uint32_t word = 0;
    int launched = RS_OK;
    if (int rc = launch_checked(t, "rs_pa_predict", "k_pa_assign", "a row", [&](uint32_t *d_err) { launched = launch_assign(t, a, d_err); }, &word)) return rc;
    if (launched) return launched;
    if (word) return fail(RS_ERR_INVALID, "rs_pa_predict: a row is not well-formed; its outputs were left as they were");
    return RS_OK;
}

int rs_pa_fit(rs_table *t, const rs_pa_metric *mt, const uint32_t *d_rows, const uint32_t *d_sel, size_t n, int n_draws, float *means, int n_means, int iterations,
              uint32_t *d_clusters, float *d_min_dist, uint32_t *changed, int *iterations_run) {
    if (int rc = check_pa("rs_pa_fit", t, mt, d_rows, n, n_draws, means, n_means)) return rc;
    if (n == 0 || n > 0xffffffffull / 47u) return fail(RS_ERR_INVALID, "rs_pa_fit: 1 .. 2^32 / 47 data");   // members[k] * 47 stays below 2^32
    if (iterations < 1 || !changed) return fail(RS_ERR_INVALID, "rs_pa_fit: iterations >= 1 and a `changed` array of that length");
    if (int rc_ = rs::table_settle(t, false)) return rc_;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    const size_t cells = size_t(n_means) * size_t(mt->n_next);
    DevBuf<float> d_means;
    DevBuf<uint32_t> d_sums, d_members, d_words, own_clusters;   // d_words: {changed, error}
    RS_HIP(d_means.alloc(cells), "rs_pa_fit: the means");
    RS_HIP(d_sums.alloc(cells), "rs_pa_fit: the sums");
    RS_HIP(d_members.alloc(size_t(n_means)), "rs_pa_fit: the member counts");
    RS_HIP(d_words.alloc(2), "rs_pa_fit: the counters");
    if (!d_clusters) {
        RS_HIP(own_clusters.alloc(n), "rs_pa_fit: the clusters");
        d_clusters = own_clusters;
    }
    RS_HIP(hipMemcpyAsync(d_means, means, cells * sizeof(float), hipMemcpyHostToDevice, t->stream), "rs_pa_fit");
    RS_HIP(hipMemsetAsync(d_clusters, 0xff, n * sizeof(uint32_t), t->stream), "rs_pa_fit");   // no cluster: the state before the first iteration
    PaAssign a = assign_args(mt, d_rows, d_sel, n, n_draws, d_means, n_means);
    a.clusters = d_clusters;
    a.min_dist = d_min_dist;
    a.changed = d_words;
    bool bad_row = false;
    int it = 0;
    for (; it < iterations; ++it) {
        RS_HIP(hipMemsetAsync(d_words, 0, 2 * sizeof(uint32_t), t->stream), "rs_pa_fit");
        RS_HIP(hipMemsetAsync(d_sums, 0, cells * sizeof(uint32_t), t->stream), "rs_pa_fit");
        RS_HIP(hipMemsetAsync(d_members, 0, size_t(n_means) * sizeof(uint32_t), t->stream), "rs_pa_fit");
        if (int rc = launch_assign(t, a, d_words + 1)) return rc;
        RS_HIP(hipGetLastError(), "k_pa_assign");
        const unsigned blocks = (unsigned)std::min<size_t>((n + kSumThreads / 64 - 1) / (kSumThreads / 64), 1u << 16);
        hipLaunchKernelGGL(k_pa_sums, dim3(blocks), dim3(kSumThreads), 0, t->stream, d_rows, d_sel, n, (const uint32_t *)d_clusters, uint32_t(n_means),
                           uint32_t(mt->n_next), d_sums.get(), d_members.get());
        RS_HIP(hipGetLastError(), "k_pa_sums");
        hipLaunchKernelGGL(k_pa_means, dim3((unsigned)std::min<size_t>((cells + kSumThreads - 1) / kSumThreads, 1u << 16)), dim3(kSumThreads), 0, t->stream,
                           (const uint32_t *)d_sums.get(), (const uint32_t *)d_members.get(), cells, uint32_t(mt->n_next), uint32_t(n_draws), d_means.get());
        RS_HIP(hipGetLastError(), "k_pa_means");
        uint32_t words[2] = {0, 0};
        RS_HIP(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, t->stream), "rs_pa_fit");
        RS_HIP(hipStreamSynchronize(t->stream), "rs_pa_fit");
        // a datum whose row is not well-formed stays in no cluster and never counts as changed after the first iteration; in the first it is one of the n
        changed[it] = it == 0 ? uint32_t(n) : words[0];
        bad_row = bad_row || words[1] != 0;
        if (changed[it] == 0) {
            ++it;
            break;
        }
    }
    if (iterations_run) *iterations_run = it;
    RS_HIP(hipMemcpyAsync(means, d_means, cells * sizeof(float), hipMemcpyDeviceToHost, t->stream), "rs_pa_fit");
    RS_HIP(hipStreamSynchronize(t->stream), "rs_pa_fit");
    if (bad_row) return fail(RS_ERR_INVALID, "rs_pa_fit: a row is not well-formed; it belongs to no cluster");
    return RS_OK;
}

}  // extern "C"
