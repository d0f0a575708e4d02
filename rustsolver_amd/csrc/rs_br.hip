// rs_br.hip -- the readers of the AVERAGE strategy.
//
//  * rs_calc_br: MCCFRTrainer::calc_br exactly as coded (cfr.rs:629-745), the two numbers train() prints at every discount
//    tick (cfr.rs:244-246).  Its `op` vectors have length 1, so of the n_buckets final strategies abstract_br_infoset collects
//    (cfr.rs:669-672) only bucket 0 of every action node is used: ONE kernel gathers get_final_strategy() of lane 0 of every node
//    (the table stays in HBM, n_nodes x 8 floats come back), and the walk itself -- a handful of f32 operations per tree node -- runs
//    on the host in the reference's operation order.
//  * rs_best_response: what that placeholder stands in for: the value of a best response to the opponent's average strategy in the
//    abstracted game (and, mode RS_BR_AVERAGE, the value of the average strategy profile itself), in vector form over the two hand
//    ranges of a single-round game on a full board -- the configuration the reference ships (options::default_flop()).  Reach and
//    value vectors live on the device as f64; every sum runs in a fixed order, so the CPU oracle reproduces the result bit for bit.
//  * rs_range_cfr_*: full-width CFR over the hand ranges on the same walk (the opponent plays the current strategy, the traverser's own nodes keep their info sets' sums as
//    regrets): three more job kinds of the best response's job table and launcher.  RS_BR_CURRENT hands the readers the regret array.
//  * rs_range_cfr_set_gadget: the re-solving gadget above the root of a full-width solver's tree (safe subgame re-solving): two more job kinds.
//  * rs_range_cfr_set_gadget_kind: the max-margin gadget in the same two places of the plan (two launches each); rs_best_response_hands: the root's value and mass rows
//    folded per hand behind one traverser's walk, one more job kind.
//  * rs_node_locks: a player's per-hand strategy fixed at chosen action nodes: the locks' rows live with the prepared game, a locked node takes two more
//    job kinds in place of its reach and value jobs, in all three walks.
//  * rs_rake: raked pots: the tree's terminals pay three numbers (win, tie, lose) instead of +-value and 0 -- no new job kind, the leaf kernels are
//    templates on RAKED and a raked run's leaf jobs go to the raked instantiations, in all three walks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <memory>
#include <vector>

#include "rs_internal.hpp"
#include "rs_device.hpp"
#include "rs_eval.hpp"

#pragma clang fp contract(off)

using namespace rs;

#define RS_HIP(call, what)                                   \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return rs::hip_fail(e_, what); \
    } while (0)

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

static unsigned grid1(uint32_t n) { return (n + kBrBlock - 1) / kBrBlock ? (n + kBrBlock - 1) / kBrBlock : 1; }
// the kernel's instantiation for the table's cell type
#define RS_BR_PICK(dtype_, K) ((dtype_) == RS_I32 ? K<kDT_I32> : ((dtype_) == RS_F32 ? K<kDT_F32> : K<kDT_F16>))

// ---- host side of calc_br: cfr.rs:640-745 over the gathered bucket-0 strategies -------------------------------------------------
struct Pay { float v[2]; };   // res[player][0]
struct AsCoded {
    const std::vector<rs_tree_node> &nodes;
    const std::vector<float> &prob;   // [index][RS_MAX_ACTIONS]
    Pay terminal(const rs_tree_node &tn, const float (&op)[2]) const {   // cfr.rs:695-745
        Pay res{{0.0f, 0.0f}};
        const float money_f = float(tn.value);
        for (int p = 0; p < 2; ++p) {
            const int opp = 1 - p;
            float opp_ges = 0.0f;
            float payoff;
            if (tn.ttype == RS_TERM_UNCONTESTED) payoff = op[opp] * (p == int(tn.last_to_act) ? -1.0f : 1.0f) * money_f;   // cfr.rs:712
            else payoff = op[opp] * money_f;                                                                                // cfr.rs:726
            res.v[p] += payoff;
            opp_ges += op[opp];
            res.v[p] *= 1.0f / opp_ges;                                                                                     // cfr.rs:716 / :730
        }
        return res;
    }
    Pay walk(int id, const float (&op)[2]) const {
        const rs_tree_node &n = nodes[size_t(id)];
        if (n.kind == RS_NODE_TERMINAL) return terminal(n, op);
        if (n.kind != RS_NODE_ACTION) return walk(n.children[0], op);   // cfr.rs:646-651: both chance kinds go to child 0
        Pay pay[RS_MAX_ACTIONS];
        const int player = n.player, opp = 1 - n.player;
        for (int a = 0; a < n.n_children; ++a) {
            float newop[2] = {op[0], op[1]};
            newop[player] *= prob[size_t(n.index) * RS_MAX_ACTIONS + size_t(a)];   // cfr.rs:677-679
            pay[a] = walk(n.children[a], newop);
        }
        float max_val = pay[0].v[player];
        int max_index = 0;
        for (int a = 1; a < n.n_children; ++a)
            if (max_val < pay[a].v[player]) {   // cfr.rs:686
                max_val = pay[a].v[player];
                max_index = a;
            }
        Pay res{{0.0f, 0.0f}};
        res.v[player] = max_val;
        res.v[opp] = pay[max_index].v[opp];
        return res;
    }
};

static int check_tree_against_table(const rs_table *t, const rs_tree *tree, const char *fn) {
    for (const rs_tree_node &n : tree->nodes) {
        if (n.kind != RS_NODE_ACTION) continue;
        if (n.index < 0 || size_t(n.index) >= t->nodes.size()) return fail(RS_ERR_INVALID, std::string(fn) + ": the tree has an action node the table lacks");
        const rs_node_desc &nd = t->nodes[size_t(n.index)];
        if (int(nd.n_actions) != n.n_children || nd.n_actions == 0 || nd.n_actions > RS_MAX_ACTIONS)
            return fail(RS_ERR_INVALID, std::string(fn) + ": action counts of tree and table differ at node " + std::to_string(n.index));
        if (nd.n_clusters == 0) return fail(RS_ERR_OOB, std::string(fn) + ": node " + std::to_string(n.index) + " has no bucket 0 (Rust: index out of bounds)");
    }
    return RS_OK;
}

static BrNodeRow row_of(const rs_table *t, int index) {
    // rows are tile[] elements apart inside the first tile of a (possibly tiled) node block: all that bucket 0 / a one-board table ever touches
    return BrNodeRow{uint64_t(t->cell_off[size_t(index)]), uint32_t(t->tile[size_t(index)]), t->nodes[size_t(index)].n_actions};
}

}  // namespace rs

extern "C" {

int rs_calc_br(rs_table *t, const rs_tree *tree, float *out) {
    if (!t || !tree || !out) return fail(RS_ERR_INVALID, "rs_calc_br: NULL argument");
    if (tree->nodes.empty()) return fail(RS_ERR_INVALID, "rs_calc_br: empty tree");
    if (int rc = check_tree_against_table(t, tree, "rs_calc_br")) return rc;
    if (int rc = table_settle(t)) return rc;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    const uint32_t n_nodes = uint32_t(t->nodes.size());
    std::vector<BrNodeRow> rows(n_nodes);
    for (uint32_t n = 0; n < n_nodes; ++n) rows[n] = row_of(t, int(n));
    std::vector<float> prob(size_t(n_nodes) * RS_MAX_ACTIONS);
    if (n_nodes) {
        DevBuf<BrNodeRow> d_rows;
        DevBuf<float> d_prob;
        RS_HIP(d_rows.alloc(rows.size()), "calc_br rows");
        hipError_t e = d_prob.alloc(prob.size());
        if (e == hipSuccess) e = hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(BrNodeRow), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(RS_BR_PICK(t->dtype, k_bucket0_final_strategy), dim3(grid1(n_nodes)), dim3(kBrBlock), 0, t->stream, t->d_ssum.get(), d_rows.get(), n_nodes, d_prob.get());
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(prob.data(), d_prob, prob.size() * sizeof(float), hipMemcpyDeviceToHost, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) return hip_fail(e, "rs_calc_br");
    }
    const AsCoded walk{tree->nodes, prob};
    const float op[2] = {1.0f, 1.0f};   // cfr.rs:631
    const Pay r = walk.walk(0, op);
    out[0] = r.v[0];                    // cfr.rs:633-636
    out[1] = r.v[1];
    return RS_OK;
}

}  // extern "C"

// ---- best response proper -----------------------------------------------------------------------------------------------
// Lanes are (run-out b, hand h), lane = b * n_hands + h: generate_hand (cfr.rs:100-143) completes the board to five cards before it draws the hands, every showdown
// compares seven-card hands on the FULL board and chance nodes pass through (cfr.rs:306-313), so every node carries vectors over all NB * n lanes; the betting round
// of a node only selects which cluster id a lane is looked up under.  A single-round game on a full board is NB = 1.
namespace rs {

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

// What a node asks of the device.  The kinds stand in the order of their launches within a tree depth -- reach on the way down, values on the way up -- which traces and
// br_launches() show.  A new own-node form is a body, a kind here, a line in BrRun::own_kind and a case in BrRun::launch.
// (the full-width sweep: kBrReachOwn on the way down, kBrOwnCfrWave / kBrOwnCfrThread on the way up; the node report: kBrReachOwn on the way down, and after the value
// job of a requested node kBrMass -- the leaf kernels on the node's q -- and kBrReport)
// (the re-solving gadget: kBrGadgetReach in front of the root's reach on the resolver's sweep, its TERMINATE leaf a kBrMass job on the root; kBrMass and kBrGadgetOwn behind
// the root's value job on the opponent's sweep; under RS_GADGET_MAXMARGIN the two kinds keep their places and are two launches each, and neither sweep has a kBrMass)
// (rs_best_response_hands: kBrMass and kBrHands behind the root's value job)
// (node locks: a locked node takes kBrLockReach where it would take a reach kind -- the opponent's q, and the traverser's pi where that goes down -- and kBrLockValue where it
// would take an own-node kind; they sort with those: the last reach kind in front of kBrLeaf, the last own-node kind in front of kBrSum)
enum BrKind { kBrGadgetReach, kBrReachGrouped, kBrReach, kBrReachOwn, kBrLockReach, kBrLeaf, kBrOwnWave, kBrOwnCols, kBrOwnGrouped, kBrOwnReal, kBrOwnCfrWave, kBrOwnCfrThread,
              kBrOwnThread, kBrLockValue, kBrSum, kBrMass, kBrReport, kBrGadgetOwn, kBrHands, kBrKinds };
// launched round by round (the round's groups, or its run-outs per prefix, shape the grid); every other kind takes the jobs of all rounds in one launch
static bool br_per_round(BrKind k) { return k == kBrReachGrouped || k == kBrOwnGrouped || k == kBrOwnReal || k == kBrReport; }
// P, Pc, O and Q of br_terminal_sorted_body
static size_t br_sorted_leaf_lds(uint32_t n_o) { return (size_t(n_o) * 2 + 52 * kBrCardHolders + 65) * sizeof(double); }
// a wave per info set (k_br_own_wave_jobs), where info sets hold many lanes
static bool br_wave_per_info_set(uint32_t lanes, uint32_t n_clusters) { return size_t(lanes) >= size_t(n_clusters) * 32; }
static uint32_t br_wave_blocks(uint32_t n_clusters) { return uint32_t(std::min<size_t>((size_t(n_clusters) * 64 + kBrBlock - 1) / kBrBlock, 8192)); }
// what a leaf is worth to traverser p before the showdown decides the sign: tn.value as f32 (cfr.rs:316); UNCONTESTED -pot for the folder, +pot for the other (cfr.rs:314-348)
static double br_terminal_value(const rs_tree_node &n, int p) {
    const double pot = double(float(n.value));
    return n.ttype == RS_TERM_UNCONTESTED && p == int(n.last_to_act) ? -pot : pot;
}

constexpr size_t kBrLevelPlanBytes = size_t(96) << 30;   // the level plan's workspace is kept with the object: not beyond 96 GB (a third of the card; 16 GB until round 5, when
                                                         // the plan bought launches only -- since the leaf loop it halves the terminals' traffic, and full 1 176-combo ranges need 59 GB)

struct BrSide {
    uint32_t n_hands = 0;
    uint32_t n = 0, n_pad = 0;     // lanes = NB * n_hands
    uint32_t n_clusters[RS_MAX_ROUNDS] = {0, 0, 0};
    uint64_t *d_mask = nullptr;    // [n_hands]
    uint32_t *d_score = nullptr;   // [n]
    uint32_t *d_cid[RS_MAX_ROUNDS] = {nullptr, nullptr, nullptr}, *d_start[RS_MAX_ROUNDS] = {nullptr, nullptr, nullptr}, *d_order[RS_MAX_ROUNDS] = {nullptr, nullptr, nullptr};
    BrGroups groups[RS_MAX_ROUNDS] = {};   // own nodes by groups of run-outs (k_br_own_grouped_jobs), where the round's info sets stay within a few run-outs each
    bool grouped[RS_MAX_ROUNDS] = {false, false, false};
    uint32_t *d_tord[RS_MAX_ROUNDS] = {nullptr, nullptr, nullptr}, *d_perm[RS_MAX_ROUNDS] = {nullptr, nullptr, nullptr};   // own nodes by columns (k_br_own_cols_jobs)
    uint32_t n_sets[RS_MAX_ROUNDS] = {0, 0, 0}, kmax[RS_MAX_ROUNDS] = {0, 0, 0};
    size_t group_lds[RS_MAX_ROUNDS] = {0, 0, 0};
    double *d_init_q = nullptr;    // this side's lanes as the OPPONENT's initial reach (its share of the deal probability)
    double *d_pw = nullptr;        // this side's lanes as the TRAVERSER's weight
    uint8_t *d_hands = nullptr;    // [n_hands][2]
    BrIndex index;                 // RS_BR_SORTED: this side as the TRAVERSER against the other side's sorted hands
};

struct BrRun {
    size_t dev_bytes = 0;                     // the ledger of its device buffers: dalloc's (the game-only half) and the walk's workspace (br_held_bytes)
    rs_table *t = nullptr;
    const rs_tree *tree = nullptr;
    int mode = RS_BR_MAX;
    bool sorted = false;           // RS_BR_SORTED: showdowns by rank order
    bool real = false;             // RS_BR_REAL (this call): the traverser's info sets are (prefix, hand), its own nodes go to k_br_own_real_*
    bool current = false;          // RS_BR_CURRENT (this call): get_strategy of the regrets where the walk reads a strategy
    bool raked = false;            // rs_rake with rate > 0 and cap > 0: the tree's terminals pay by rs_rake_payoffs and their leaf jobs go to the RAKED kernels
    rs_rake rake{};                // ... the rake, as given
    bool cfr = false;              // the object is a full-width solver's (br_cfr_sweep): pi buffers in the workspace, own nodes go to k_br_cfr_own*
    int cfr_rmplus = 0;            // ... RS_UPD_RMPLUS of the sweep in flight
    double *d_pi0[2] = {nullptr, nullptr};    // ... the traverser's own reach at the root: 1.0 on every lane (the node report's as well)
    const std::vector<int> *report_slot = nullptr;   // the node report in flight (br_report): per tree node its place in the request, -1 = not asked for
    const uint64_t *report_off = nullptr;     // ... where every requested node's block starts in d_report
    double *d_report = nullptr;               // ... the call's output buffer on the device
    bool ws_pi = false;                       // the workspace has the own-reach rows (a full-width solver's, or one a report has walked on)
    size_t ws_mass_rows = 0;                  // ... and this many mass rows in the level plan (one per depth otherwise)
    std::vector<double *> mass_level;         // ... per tree depth (depth-first walk)
    // the re-solving gadget of a full-width solver (br_cfr_set_gadget): the resolver (-1 = none), alt[n], the f32 rows regret[2][n] and ssum[2][n] of the opponent's n hands,
    // the opponent's two scaled reach rows (FOLLOW, TERMINATE) and per side one extra lane row: the mass row on the opponent's sweep, the TERMINATE leaf's on the resolver's
    int gadget = -1;
    double *d_g_alt = nullptr, *d_g_qf = nullptr, *d_g_qt = nullptr, *d_g_row[2] = {nullptr, nullptr};
    float *d_g_regret = nullptr, *d_g_ssum = nullptr;
    // RS_GADGET_MAXMARGIN (br_cfr_set_gadget's kind 1; the buffers come with the first arming of that kind): per opponent hand F (the root row's fold of the last
    // opponent's sweep), M (the root mass row's fold: the game's alone, computed once per arming by br_mm_mass), rho / M and the margins; d_g_out = {U, sum of rho * alt}
    int gadget_kind = RS_GADGET_RESOLVE;
    double *d_g_F = nullptr, *d_g_M = nullptr, *d_g_scale = nullptr, *d_g_margin = nullptr, *d_g_out = nullptr;
    bool g_M_ready = false, g_margin_ready = false;
    double g_out[2] = {0.0, 0.0};             // ... d_g_out of the last sweep, on the host
    // rs_best_response_hands in flight (br_hands): the root's mass row [n_pad] and the output [2][n_hands of the traverser] on the device, nullptr otherwise
    double *d_hands_mass = nullptr, *d_hands_out = nullptr;
    // node locks (rs_node_locks): per tree node its lock's rows [A][prefixes of its round][hands of the acting player] on the device (dalloc: the game-only half), nullptr =
    // not locked; empty when the game has no lock at all
    std::vector<const double *> lock_of;
    const double *lock_at(size_t id) const { return lock_of.empty() ? nullptr : lock_of[id]; }
    bool takes_pi() const { return cfr || report_slot; }   // the traverser's own reach goes down beside q
    uint32_t per_prefix[RS_MAX_ROUNDS] = {1, 1, 1};   // run-outs under a prefix of round r
    int p = 0;
    uint32_t NB = 1;
    int n_board0 = 5;              // cards of the initial board
    uint64_t *d_bmask = nullptr;
    BrSide side[2];
    std::vector<DevBuf<char>> allocs;
    std::vector<double *> q_level, v_level;   // per tree depth: [max actions][n_pad] children buffers
    std::vector<double *> pi_level;           // ... and the traverser's own reach (full-width sweep)
    double *d_root = nullptr;                 // [n_pad_max]: the root values of the traverser's lanes (depth-first walk)
    bool last_level_plan = false;             // what the last br_execute ran, and its launches (level plan)
    int last_launches = 0;
    DevBuf<double> ws;                        // the walk's workspace, allocated by the first br_execute and kept (a 60 GB allocation takes seconds): level plan or depth-first
    bool ws_levels = false;
    DevBuf<BrJob> job_table;                  // a traverser's jobs on the device: kept with the workspace and grown when a plan holds more (an allocation per pass costs a
                                              // launch-bound sweep a fifth of its time, profiles/br_launcher.md); like the per-pass table it replaces, not in the ledger
    void release_workspace() {
        if (ws) (void)hipStreamSynchronize(t->stream);
        ws.reset();
        job_table.reset();
        q_level.clear();
        v_level.clear();
        pi_level.clear();
        mass_level.clear();
        ws_pi = false;
        ws_mass_rows = 0;
        d_root = nullptr;
    }
    size_t n_pad_max = 0;
    hipError_t err = hipSuccess;

    template <typename T> T *dalloc(size_t n) {
        DevBuf<char> b;
        if (err == hipSuccess) err = b.alloc(std::max<size_t>(n, 1) * sizeof(T), &dev_bytes);
        T *ptr = reinterpret_cast<T *>(b.get());
        if (ptr) allocs.push_back(std::move(b));
        return ptr;
    }
    template <typename T> T *upload(const std::vector<T> &h) {
        T *d = dalloc<T>(h.size());
        if (err == hipSuccess && !h.empty()) err = hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);   // blocking: h may be a temporary
        return d;
    }

    // ---- the two tree orders.  The LEVEL PLAN gives every node buffers of its own (an action node: [A][n_pad] for its children's values, an opponent's node the same for
    // their reach), so the nodes of one tree depth no longer wait for each other and ONE launch takes all of a depth's nodes of one kind (grid row = node): reach down level by
    // level, every leaf in one launch, values up level by level -- about sixty launches per traverser instead of one or two per tree node (1 864 nodes: 4 300 launches per
    // call).  Costs memory: see level_plan_bytes.  The DEPTH-FIRST walk shares two buffers per tree depth among the depth's nodes and launches node by node.  Both run the
    // same jobs through the same kernels (build_plan, launch), so their bits are the same.
    int max_depth = 0;            // action nodes on the longest path: the levels of child buffers
    std::vector<int> depth_of;    // per tree node: action-node ancestors
    void fill_depths() {
        depth_of.assign(tree->nodes.size(), 0);
        max_depth = 0;
        for (size_t id = 0; id < tree->nodes.size(); ++id) {   // parents come before children
            const rs_tree_node &n = tree->nodes[id];
            for (int a = 0; a < n.n_children; ++a) depth_of[size_t(n.children[a])] = depth_of[id] + (n.kind == RS_NODE_ACTION ? 1 : 0);
            if (n.kind == RS_NODE_ACTION) max_depth = std::max(max_depth, depth_of[id] + 1);
        }
    }
    size_t level_plan_bytes(int pl, bool pi, size_t mass_rows) const {   // workspace of traverser pl's pass
        const BrSide &me = side[pl], &op = side[1 - pl];
        size_t doubles = me.n_pad + mass_rows * me.n_pad;   // the root vector; a mass row per node a report asks for
        for (const rs_tree_node &n : tree->nodes)
            if (n.kind == RS_NODE_ACTION && n.n_children > 0)   // children's values; an opponent node their reach as well, an own node their pi (full-width sweep, node report)
                doubles += size_t(n.n_children) * (size_t(me.n_pad) + (int(n.player) != pl ? size_t(op.n_pad) : (pi ? size_t(me.n_pad) : 0)));
        return doubles * sizeof(double);
    }

    // which kernel takes the traverser's own nodes of round r / the opponent's: groups and columns are the level plan's only
    BrKind own_kind(int r) const {
        const BrSide &me = side[p];
        if (cfr) return br_wave_per_info_set(me.n, me.n_clusters[r]) ? kBrOwnCfrWave : kBrOwnCfrThread;   // (no groups, no columns: a follow-up once a profile asks)
        if (real) return kBrOwnReal;   // whatever the abstraction's lists would have asked for
        if (ws_levels && mode == RS_BR_MAX && me.grouped[r]) return kBrOwnGrouped;
        if (ws_levels && me.d_tord[r]) return kBrOwnCols;
        return br_wave_per_info_set(me.n, me.n_clusters[r]) ? kBrOwnWave : kBrOwnThread;
    }
    BrKind reach_kind(int r) const { return !cfr && ws_levels && side[1 - p].grouped[r] ? kBrReachGrouped : kBrReach; }

    // One traverser's pass as jobs in the order of their launches: reach by ascending depth, the leaves, values by descending depth, within a depth by kind (and round, where
    // the kind is launched per round).  A run of equal `key` is one launch of the level plan.
    struct BrPlan {
        struct Entry {
            uint32_t key;
            BrKind kind;
            int round, node;
        };
        std::vector<Entry> entries;
        std::vector<BrJob> jobs;           // jobs[i] is entries[i]'s
        std::vector<int> job_at, sum_at;   // per tree node: its job (leaf, own node, an opponent node's reach) and an opponent node's sum job, -1 = none
        std::vector<int> own_reach_at;     // ... an own node's reach job (full-width sweep, node report)
        std::vector<int> mass_at, report_at;   // ... a requested node's mass and report jobs (node report)
        int gadget_reach_at = -1, gadget_mass_at = -1, gadget_own_at = -1;   // the gadget's jobs above the root (a full-width solver with a gadget)
        int hands_at = -1;                 // rs_best_response_hands' fold of the root rows (its root mass job sits in gadget_mass_at)
        double *root = nullptr;            // where the root's values arrive
    };
    // host only: gives every node its buffers and fills the jobs
    int build_plan(BrPlan &pl) {
        const BrSide &me = side[p], &op = side[1 - p];
        const size_t N = tree->nodes.size();
        double *at = ws;
        auto slot = [&](size_t doubles) {   // level plan: the next stretch of the workspace
            double *s = at;
            at += doubles;
            return s;
        };
        pl.root = ws_levels ? slot(me.n_pad) : d_root;
        std::vector<const double *> q_in(N, nullptr), pi_in(N, nullptr);
        std::vector<double *> v_out(N, nullptr);
        std::vector<int> folds(N, -1);   // an own node whose kernel adds up the rows below an opponent's child itself (by groups, real game; level plan): its job
        v_out[0] = pl.root;
        q_in[0] = op.d_init_q;
        pi_in[0] = d_pi0[p];
        std::vector<BrPlan::Entry> entries;   // in the tree's order; gathered into pl in launch order below
        std::vector<BrJob> jobs;
        auto add = [&](BrKind kind, int r, size_t id, const BrJob &j) {
            const int d = depth_of[id], step = kind < kBrLeaf ? d : (kind == kBrLeaf ? max_depth + 1 : 2 * max_depth + 2 - d);
            entries.push_back({(uint32_t(step) * kBrKinds + kind) * RS_MAX_ROUNDS + uint32_t(br_per_round(kind) ? r : 0), kind, r, int(id)});
            jobs.push_back(j);
        };
        auto lock_reach = [&](const double *lock, int r, const BrSide &s, const double *in, double *out, uint32_t n_children) {   // a kBrLockReach job on side s's lanes
            BrJob jl{};
            jl.sum_src[0] = lock;
            jl.n_clusters = per_prefix[r];
            jl.n_sets = s.n_hands;
            jl.kmax = s.n;
            jl.row.pitch = s.n_pad;
            jl.q = in;
            jl.q_out = out;
            jl.n_children = n_children;
            return jl;
        };
        if (cfr && gadget >= 0) {   // the gadget node above the root; its rows belong to the object, not to the workspace
            BrJob jm{};
            jm.v = d_g_row[p];
            jm.uncontested = 1;
            if (p == gadget) {   // the resolver's sweep: the opponent enters the tree with its FOLLOW share, the rest meets the TERMINATE leaf
                BrJob jg{};
                jg.q = op.d_init_q;
                jg.q_out = d_g_qf;
                jg.v = d_g_qt;
                add(kBrGadgetReach, 0, 0, jg);
                q_in[0] = d_g_qf;
                jm.q = d_g_qt;
                jm.value = -1.0;
                if (gadget_kind == RS_GADGET_RESOLVE) add(kBrMass, 0, 0, jm);   // (max-margin has no TERMINATE leaf: the hand choice sits in the opponent's reach)
            } else {             // the opponent's sweep: the root's mass row, then the gadget's own node over the root row
                jm.q = op.d_init_q;
                jm.value = 1.0;
                if (gadget_kind == RS_GADGET_RESOLVE) add(kBrMass, 0, 0, jm);   // (max-margin reads M, folded once per arming: br_mm_mass)
                BrJob jo{};
                jo.v = pl.root;
                jo.sum_src[0] = d_g_row[p];
                add(kBrGadgetOwn, 0, 0, jo);
            }
        }
        if (d_hands_out) {   // rs_best_response_hands: the root's mass row and the fold of both root rows, behind the root's value job in either tree order
            BrJob jm{};
            jm.q = op.d_init_q;
            jm.v = d_hands_mass;
            jm.uncontested = 1;
            jm.value = 1.0;
            add(kBrMass, 0, 0, jm);
            BrJob jf{};
            jf.v = pl.root;
            jf.sum_src[0] = d_hands_mass;
            jf.q_out = d_hands_out;
            add(kBrHands, 0, 0, jf);
        }
        for (size_t id = 0; id < N; ++id) {   // parents before children: a node's q and v slot are known when it comes up
            const rs_tree_node &n = tree->nodes[id];
            if (n.kind == RS_NODE_TERMINAL) {
                BrJob j{};
                j.q = q_in[id];
                j.v = v_out[id];
                j.uncontested = n.ttype == RS_TERM_UNCONTESTED;
                j.value = br_terminal_value(n, p);
                if (raked) {   // the one place the formulas live: win, tie, lose (an uncontested leaf: its one payoff three times)
                    double pay[3];
                    if (int rc = rs_rake_payoffs(tree, int(id), &rake, p, pay)) return rc;
                    j.value = pay[0], j.value_tie = pay[1], j.value_lose = pay[2];
                }
                add(kBrLeaf, 0, id, j);
                continue;
            }
            if (n.kind != RS_NODE_ACTION) {   // chance nodes pass through (cfr.rs:306-313)
                if (n.n_children > 0) {
                    q_in[size_t(n.children[0])] = q_in[id];
                    pi_in[size_t(n.children[0])] = pi_in[id];
                    v_out[size_t(n.children[0])] = v_out[id];
                }
                continue;
            }
            if (n.n_children == 0) return fail(RS_ERR_UNSUPPORTED, "rs_best_response: an action node without actions");
            const int r = n.round_idx, d = depth_of[id];
            BrJob j{};
            j.row = row_of(t, n.index);
            double *vch = ws_levels ? slot(size_t(n.n_children) * me.n_pad) : v_level[size_t(d)];
            j.vch = vch;
            j.v = v_out[id];
            j.n_children = uint32_t(n.n_children);
            const double *const lock = lock_at(id);
            if (lock && int(n.player) == p) {   // a locked own node: its value by the lock, never a fold, nothing of the table read -- its opponent children get their kBrSum jobs
                j.sum_src[0] = lock;
                j.n_clusters = per_prefix[r];
                if (takes_pi()) {
                    double *pch = ws_levels ? slot(size_t(n.n_children) * me.n_pad) : pi_level[size_t(d)];
                    add(kBrLockReach, r, id, lock_reach(lock, r, me, pi_in[id], pch, j.n_children));
                    j.q = pi_in[id];
                    for (int a = 0; a < n.n_children; ++a) pi_in[size_t(n.children[a])] = pch + size_t(a) * me.n_pad;
                }
                add(kBrLockValue, r, id, j);
                for (int a = 0; a < n.n_children; ++a) q_in[size_t(n.children[a])] = q_in[id];
            } else if (int(n.player) == p) {
                const BrKind kind = own_kind(r);
                j.start = me.d_start[r];
                j.order = me.d_order[r];
                j.n_clusters = me.n_clusters[r];
                if (kind == kBrOwnCols) {
                    j.tord = me.d_tord[r];
                    j.perm = me.d_perm[r];
                    j.n_sets = me.n_sets[r];
                    j.kmax = me.kmax[r];
                }
                if (ws_levels && (kind == kBrOwnGrouped || kind == kBrOwnReal)) folds[id] = int(jobs.size());
                if (takes_pi()) {   // its children's pi on the way down; the update (the report) reads the pi that came in
                    double *pch = ws_levels ? slot(size_t(n.n_children) * me.n_pad) : pi_level[size_t(d)];
                    BrJob jr{};
                    jr.row = j.row;
                    jr.cid = me.d_cid[r];
                    jr.q = pi_in[id];
                    jr.q_out = pch;
                    jr.n_children = j.n_children;
                    add(kBrReachOwn, r, id, jr);
                    j.q = pi_in[id];
                    for (int a = 0; a < n.n_children; ++a) pi_in[size_t(n.children[a])] = pch + size_t(a) * me.n_pad;
                }
                add(kind, r, id, j);
                for (int a = 0; a < n.n_children; ++a) q_in[size_t(n.children[a])] = q_in[id];
            } else {
                double *qch = ws_levels ? slot(size_t(n.n_children) * op.n_pad) : q_level[size_t(d)];
                j.cid = op.d_cid[r];
                j.q = q_in[id];
                j.q_out = qch;
                // a locked opponent node: its children's reach by the lock; its value stays the sum of theirs (kBrSum below, or the parent's fold)
                if (lock) add(kBrLockReach, r, id, lock_reach(lock, r, op, q_in[id], qch, j.n_children));
                else add(reach_kind(r), r, id, j);
                // its value is the sum of its children's; where the parent folds, that kernel adds the rows up as it loads them
                const int par = n.parent;
                bool taken = false;
                if (par >= 0 && folds[size_t(par)] >= 0) {
                    const rs_tree_node &pn = tree->nodes[size_t(par)];
                    BrJob &pj = jobs[size_t(folds[size_t(par)])];
                    for (int a = 0; a < pn.n_children && !taken; ++a)
                        if (pn.children[a] == int(id)) {
                            pj.sum_src[a] = vch;
                            pj.sum_n[a] = uint32_t(n.n_children);
                            taken = true;
                        }
                }
                if (!taken) add(kBrSum, r, id, j);
                for (int a = 0; a < n.n_children; ++a) q_in[size_t(n.children[a])] = qch + size_t(a) * op.n_pad, pi_in[size_t(n.children[a])] = pi_in[id];
            }
            for (int a = 0; a < n.n_children; ++a) v_out[size_t(n.children[a])] = vch + size_t(a) * me.n_pad;
            if (report_slot && (*report_slot)[id] >= 0) {   // after the node's value job (kinds sort behind kBrSum within the node's step): its buffers are alive in both orders
                double *mass = ws_levels ? slot(me.n_pad) : mass_level[size_t(d)];
                BrJob jm{};
                jm.q = q_in[id];
                jm.v = mass;
                jm.uncontested = 1;
                jm.value = 1.0;
                add(kBrMass, r, id, jm);
                BrJob jr{};
                jr.vch = vch;
                jr.v = v_out[id];
                jr.n_children = uint32_t(n.n_children);
                jr.q = pi_in[id];
                jr.sum_src[0] = mass;
                jr.q_out = d_report + report_off[size_t((*report_slot)[id])];
                add(kBrReport, r, id, jr);
            }
        }
        // into launch order; within a launch the nodes keep the tree's order
        std::vector<uint32_t> perm(entries.size());
        for (uint32_t i = 0; i < perm.size(); ++i) perm[i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return entries[a].key < entries[b].key; });
        pl.job_at.assign(N, -1);
        pl.sum_at.assign(N, -1);
        pl.own_reach_at.assign(N, -1);
        pl.mass_at.assign(N, -1);
        pl.report_at.assign(N, -1);
        pl.entries.reserve(perm.size());
        pl.jobs.reserve(perm.size());
        for (uint32_t i : perm) {
            const BrPlan::Entry &e = entries[i];
            if (e.kind == kBrGadgetReach || e.kind == kBrGadgetOwn || e.kind == kBrHands || (e.kind == kBrMass && (cfr || d_hands_out))) {
                // (a full-width solver's only mass job is the gadget's, a per-hand walk's only one the root's)
                (e.kind == kBrGadgetReach ? pl.gadget_reach_at : (e.kind == kBrGadgetOwn ? pl.gadget_own_at : (e.kind == kBrHands ? pl.hands_at : pl.gadget_mass_at))) =
                    int(pl.jobs.size());
                pl.entries.push_back(e);
                pl.jobs.push_back(jobs[i]);
                continue;
            }
            const bool own_reach = e.kind == kBrReachOwn || (e.kind == kBrLockReach && int(tree->nodes[size_t(e.node)].player) == p);   // (a locked opponent node's reach is its job)
            std::vector<int> &at_of = e.kind == kBrSum ? pl.sum_at : (own_reach ? pl.own_reach_at : (e.kind == kBrMass ? pl.mass_at : (e.kind == kBrReport ? pl.report_at : pl.job_at)));
            at_of[size_t(e.node)] = int(pl.jobs.size());
            pl.entries.push_back(e);
            pl.jobs.push_back(jobs[i]);
        }
        return RS_OK;
    }

    // The launcher: for every kind the ONE place that knows its grid, block and LDS size, its attributes, the instantiation for the cell type and the leaf form.  d_jobs[0 .. nj)
    // are the launch's jobs (one grid row each), h the same jobs on the host; r is the round of a kind that is launched per round.  The level plan passes a run of equal key,
    // the depth-first walk one row of the same table: the same kernels with a one-row grid (timed against one-node entries in profiles/br_launcher.md; kBrOwnWave kept its own).
    int n_launches = 0;
    void launch(BrKind kind, int r, const BrJob *d_jobs, uint32_t nj, const BrJob *h) {
        if (err != hipSuccess) return;
        const BrSide &me = side[p], &op = side[1 - p];
        const hipStream_t s = t->stream;
        const void *ssum = (current || cfr) ? t->d_regrets.get() : t->d_ssum.get();   // what the strategy readers read: the average strategy's array or the current one's
        float *const cfr_regrets = reinterpret_cast<float *>(t->d_regrets.get()), *const cfr_ssum = reinterpret_cast<float *>(t->d_ssum.get());   // the full-width update's
        const dim3 block(kBrBlock);
        auto most = [&](auto field) {   // the grid is sized by the largest of the launch's jobs
            uint32_t m = 0;
            for (uint32_t i = 0; i < nj; ++i) m = std::max<uint32_t>(m, field(h[i]));
            return m;
        };
        auto n_clusters = [](const BrJob &j) { return j.n_clusters; };
        switch (kind) {
        case kBrReachGrouped: {
            const BrGroups &g = op.groups[r];
            const size_t lds = size_t(most([](const BrJob &j) { return j.row.n_actions; })) * (size_t(g.max_sets) + 1) * sizeof(float);
            const auto k = RS_BR_PICK(t->dtype, k_br_opp_reach_grouped_jobs);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
            hipLaunchKernelGGL(k, dim3(8u * ((g.n_groups + 7u) / 8u), nj), dim3(kBrGroupBlock), lds, s, ssum, d_jobs, g, op.n_pad);
            break;
        }
        case kBrReach: {
            const auto k = RS_BR_PICK(t->dtype, k_br_opp_reach_jobs);
            hipLaunchKernelGGL(k, dim3(8u * grid1(NB * ((op.n_hands + 7u) / 8u)), nj), block, 0, s, ssum, d_jobs, op.n, op.n_pad, op.n_hands);
            break;
        }
        case kBrReachOwn: {
            const auto k = RS_BR_PICK(t->dtype, k_br_own_reach_jobs);
            hipLaunchKernelGGL(k, dim3(8u * grid1(NB * ((me.n_hands + 7u) / 8u)), nj), block, 0, s, ssum, d_jobs, me.n, me.n_pad, me.n_hands);
            break;
        }
        case kBrMass:   // the mass row of a requested node: the leaf kernels of the run's showdown mode on the node's q
        case kBrLeaf: {
            // (small ranges keep a workgroup per (run-out, leaf): the loop's scans are unrolled for 1 326 hands whatever the range holds -- 200 combos: 0.047 against 0.059 s per call)
            const uint32_t most_hands = std::max(me.n_hands, op.n_hands);
            const bool rk = raked && kind == kBrLeaf;   // a raked run's tree terminals go to the RAKED instantiations; mass rows are no terminals (uncontested, 1.0)
            if (sorted && ws_levels && most_hands <= uint32_t(kBrHandsPerThread) * kBrBlock && op.n_hands <= uint32_t(kBrChunkMax) * 64u) {
                // the level plan's leaf loop: a workgroup per run-out (and slice of the leaves, when run-outs alone do not fill the card)
                const size_t lds = br_sorted_leaf_lds(op.n_hands) + (((size_t(op.n_hands) + 3) & ~size_t(3)) + 52 * kBrCardHolders) * sizeof(uint16_t) + 64;
                // slices of the leaves: enough workgroups to fill the card, and a count that leaves the last round of workgroups (two per CU at full ranges: 220 registers;
                // four and more for the small-range forms) nearly full -- 2 352 run-outs on 512 slots are 4.6 rounds (the fifth 59 % full), three slices 13.8
                const int form = most_hands <= 256 ? 0 : (most_hands <= 512 ? 1 : (most_hands <= 1024 ? 2 : 3));
                uint32_t slices = std::max<uint32_t>(1, std::min<uint32_t>(nj, 2048u / std::max<uint32_t>(NB, 1)));
                {
                    int cus = 256;
                    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus < 1) cus = 256;
                    const double slots = (form == 3 ? 2.0 : 4.0) * cus;
                    double best = 0.0;
                    for (uint32_t sl = slices; sl <= std::min<uint32_t>(nj, slices + 7); ++sl) {
                        const double rounds = double(NB) * sl / slots, eff = rounds / std::ceil(rounds);
                        if (eff > best + 0.02) best = eff, slices = sl;
                        if (eff >= 0.95) break;
                    }
                }
#define RS_LEAF_LOOP_(HPT_, CHUNK_, RAKED_)                                                                                                                                    \
    hipLaunchKernelGGL((k_br_terminal_sorted_loop<HPT_, CHUNK_, (HPT_ == kBrHandsPerThread), RAKED_>), dim3(NB, slices), block, lds, s, me.d_hands, me.d_mask, me.d_pw, me.n_hands, \
                       op.n_hands, d_bmask, me.index, d_jobs, nj)
#define RS_LEAF_LOOP(HPT_, CHUNK_)                                                                                                                                             \
    do {                                                                                                                                                                       \
        if (rk) RS_LEAF_LOOP_(HPT_, CHUNK_, true);                                                                                                                              \
        else RS_LEAF_LOOP_(HPT_, CHUNK_, false);                                                                                                                                \
    } while (0)
                if (form == 0) RS_LEAF_LOOP(1, 4);
                else if (form == 1) RS_LEAF_LOOP(2, 8);
                else if (form == 2) RS_LEAF_LOOP(4, 16);
                else RS_LEAF_LOOP(kBrHandsPerThread, kBrChunkMax);
#undef RS_LEAF_LOOP
#undef RS_LEAF_LOOP_
            } else if (sorted) {   // a workgroup per (run-out, leaf)
                hipLaunchKernelGGL(rk ? k_br_terminal_sorted_jobs<true> : k_br_terminal_sorted_jobs<false>, dim3(NB, nj), block, br_sorted_leaf_lds(op.n_hands), s, me.d_hands,
                                   me.d_mask, me.d_pw, me.n_hands, op.n_hands, d_bmask, me.index, d_jobs);
            } else {
                const size_t lds = size_t(op.n_hands) * (sizeof(double) + sizeof(uint64_t) + sizeof(uint32_t));
                hipLaunchKernelGGL(rk ? k_br_terminal_boards_jobs<true> : k_br_terminal_boards_jobs<false>, dim3(grid1(me.n_hands), NB, nj), block, lds, s, me.d_mask, me.d_score,
                                   me.d_pw, me.n_hands, op.d_mask, op.d_score, op.n_hands, d_bmask, d_jobs);
            }
            break;
        }
        case kBrOwnWave: {
            if (!ws_levels) {   // depth first: the kind's one-node entry (see there)
                hipLaunchKernelGGL(RS_BR_PICK(t->dtype, k_br_own_wave), dim3(br_wave_blocks(h->n_clusters)), block, 0, s, ssum, h->row, h->start, h->order, h->n_clusters, me.n_pad,
                                   h->vch, mode, h->v);
                break;
            }
            const auto k = RS_BR_PICK(t->dtype, k_br_own_wave_jobs);
            hipLaunchKernelGGL(k, dim3(br_wave_blocks(most(n_clusters)), nj), block, 0, s, ssum, d_jobs, me.n_pad, mode);
            break;
        }
        case kBrOwnCols: {
            const auto k = RS_BR_PICK(t->dtype, k_br_own_cols_jobs);
            hipLaunchKernelGGL(k, dim3(grid1(most([](const BrJob &j) { return j.n_sets; })), nj), block, 0, s, ssum, d_jobs, me.n_pad, mode);
            break;
        }
        case kBrOwnGrouped:
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_br_own_grouped_jobs), hipFuncAttributeMaxDynamicSharedMemorySize, int(me.group_lds[r]));
            hipLaunchKernelGGL(k_br_own_grouped_jobs, dim3(me.groups[r].n_groups, nj), dim3(kBrGroupBlock), me.group_lds[r], s, d_jobs, me.groups[r], me.n_pad);
            break;
        case kBrOwnReal: {
            const uint32_t pp = per_prefix[r], n_pairs = me.n / pp;
            const dim3 cols_grid((n_pairs + kBrRealPairs - 1) / kBrRealPairs, nj);
            if (pp == 1) hipLaunchKernelGGL(k_br_own_real_last_jobs, dim3(grid1(me.n), nj), block, 0, s, me.d_mask, d_bmask, me.n_hands, me.n, me.n_pad, d_jobs);
            else hipLaunchKernelGGL(k_br_own_real_cols_jobs, cols_grid, block, 0, s, me.d_mask, d_bmask, me.n_hands, n_pairs, pp, me.n_pad, d_jobs);
            break;
        }
        case kBrOwnCfrWave:
            hipLaunchKernelGGL(k_br_cfr_own_wave_jobs, dim3(br_wave_blocks(most(n_clusters)), nj), block, 0, s, cfr_regrets, cfr_ssum, d_jobs, me.n_pad, cfr_rmplus);
            break;
        case kBrOwnCfrThread:
            hipLaunchKernelGGL(k_br_cfr_own_jobs, dim3(grid1(most(n_clusters)), nj), block, 0, s, cfr_regrets, cfr_ssum, d_jobs, me.n_pad, cfr_rmplus);
            break;
        case kBrOwnThread: {
            const auto k = RS_BR_PICK(t->dtype, k_br_own_jobs);
            hipLaunchKernelGGL(k, dim3(grid1(most(n_clusters)), nj), block, 0, s, ssum, d_jobs, me.n_pad, mode);
            break;
        }
        case kBrLockReach:   // the jobs carry their side's shape: the grid is sized by the longest lane row
            hipLaunchKernelGGL(k_br_lock_reach_jobs, dim3(grid1(most([](const BrJob &j) { return j.kmax; })), nj), block, 0, s, d_jobs);
            break;
        case kBrLockValue:
            hipLaunchKernelGGL(k_br_lock_value_jobs, dim3(grid1(me.n), nj), block, 0, s, me.d_mask, d_bmask, me.n_hands, me.n, me.n_pad, d_jobs);
            break;
        case kBrSum:
            hipLaunchKernelGGL(k_br_sum_jobs, dim3(grid1(me.n), nj), block, 0, s, d_jobs, me.n, me.n_pad);
            break;
        case kBrReport: {
            const uint32_t pp = per_prefix[r], n_pairs = me.n / pp;
            const dim3 cols_grid((n_pairs + kBrRealPairs - 1) / kBrRealPairs, nj);
            if (pp == 1) hipLaunchKernelGGL(k_br_report_last_jobs, dim3(grid1(me.n), nj), block, 0, s, me.d_mask, d_bmask, me.n_hands, me.n, me.n_pad, d_jobs);
            else hipLaunchKernelGGL(k_br_report_cols_jobs, cols_grid, block, 0, s, me.d_mask, d_bmask, me.n_hands, n_pairs, pp, me.n_pad, d_jobs);
            break;
        }
        case kBrGadgetReach:   // one job, whichever tree order: the same launch
            if (gadget_kind == RS_GADGET_MAXMARGIN) {   // max-margin: rho / M per hand in one workgroup, then the per-lane scale
                hipLaunchKernelGGL(k_br_mm_scale, dim3(1), block, 0, s, d_g_regret, d_g_M, d_g_alt, op.n_hands, d_g_scale, d_g_out);
                err = hipGetLastError();
                ++n_launches;
                if (err != hipSuccess) return;
                hipLaunchKernelGGL(k_br_mm_reach, dim3(grid1(op.n)), block, 0, s, d_g_scale, op.n_hands, op.n, h->q, h->q_out);
                break;
            }
            hipLaunchKernelGGL(k_br_gadget_reach, dim3(grid1(op.n)), block, 0, s, d_g_regret, d_g_alt, op.n_hands, op.n, h->q, h->q_out, h->v);
            break;
        case kBrGadgetOwn:
            if (gadget_kind == RS_GADGET_MAXMARGIN) {   // max-margin: the fold of the root row, then the hand-level update in one workgroup
                hipLaunchKernelGGL(k_br_hands_fold, dim3(grid1(me.n_hands)), block, 0, s, me.d_mask, d_bmask, me.n_hands, NB, h->v, (const double *)nullptr, d_g_F, d_g_M);
                err = hipGetLastError();
                ++n_launches;
                if (err != hipSuccess) return;
                hipLaunchKernelGGL(k_br_mm_update, dim3(1), block, 0, s, d_g_regret, d_g_ssum, d_g_F, d_g_M, d_g_alt, me.n_hands, d_g_margin, d_g_out, cfr_rmplus);
                break;
            }
            hipLaunchKernelGGL(k_br_gadget_own, dim3(grid1(me.n_hands)), block, 0, s, me.d_mask, d_bmask, me.n_hands, NB, d_g_regret, d_g_ssum, d_g_alt, h->sum_src[0], h->v, cfr_rmplus);
            break;
        case kBrHands:
            hipLaunchKernelGGL(k_br_hands_fold, dim3(grid1(me.n_hands)), block, 0, s, me.d_mask, d_bmask, me.n_hands, NB, h->v, h->sum_src[0], h->q_out, h->q_out + me.n_hands);
            break;
        case kBrKinds:   // a count, no kind
            return;
        }
        err = hipGetLastError();
        ++n_launches;
    }

    // row `at` of the uploaded job table as a launch of its own: every launch of the depth-first order
    void one(const BrPlan &pl, int at) { launch(pl.entries[size_t(at)].kind, pl.entries[size_t(at)].round, job_table + at, 1, &pl.jobs[size_t(at)]); }
    // depth first: a node's launches around its children's
    void walk(const BrPlan &pl, int id) {
        if (err != hipSuccess) return;
        const rs_tree_node &n = tree->nodes[size_t(id)];
        if (n.kind != RS_NODE_TERMINAL && n.kind != RS_NODE_ACTION) return walk(pl, n.children[0]);   // chance nodes pass through (cfr.rs:306-313)
        const bool own = n.kind == RS_NODE_ACTION && int(n.player) == p;
        if (!own) one(pl, pl.job_at[size_t(id)]);   // a leaf, or the reach of an opponent node's children
        else if (pl.own_reach_at[size_t(id)] >= 0) one(pl, pl.own_reach_at[size_t(id)]);   // full-width sweep, node report: the traverser's own reach of its children
        if (n.kind == RS_NODE_TERMINAL) return;
        for (int a = 0; a < n.n_children; ++a) walk(pl, n.children[a]);
        one(pl, own ? pl.job_at[size_t(id)] : pl.sum_at[size_t(id)]);
        if (pl.report_at[size_t(id)] >= 0) {   // node report: while the depth's buffers are this node's
            one(pl, pl.mass_at[size_t(id)]);
            one(pl, pl.report_at[size_t(id)]);
        }
    }

    // one traverser's pass: the plan, one upload of its jobs, the launches in the tree order the workspace was made for, the root's values back
    int run_traverser(double *root_host) {
        BrPlan pl;
        if (int rc = build_plan(pl)) return rc;
        n_launches = 0;
        if (job_table.bytes() < pl.jobs.size() * sizeof(BrJob)) err = job_table.alloc(pl.jobs.size());   // (no pass is in flight: each ends with a stream synchronise)
        if (err == hipSuccess) err = hipMemcpyAsync(job_table, pl.jobs.data(), pl.jobs.size() * sizeof(BrJob), hipMemcpyHostToDevice, t->stream);
        if (!ws_levels) {   // the gadget's jobs above the root (a resolver's sweeps only), the tree between them
            if (pl.gadget_reach_at >= 0) one(pl, pl.gadget_reach_at);
            walk(pl, 0);
            if (pl.gadget_mass_at >= 0) one(pl, pl.gadget_mass_at);
            if (pl.gadget_own_at >= 0) one(pl, pl.gadget_own_at);
            if (pl.hands_at >= 0) one(pl, pl.hands_at);
        } else {   // reach downwards by depth, the leaves in slices of 16 384, values upwards by depth: the plan's order
            for (size_t lo = 0, hi; lo < pl.jobs.size() && err == hipSuccess; lo = hi) {
                const size_t most = pl.entries[lo].kind == kBrLeaf || pl.entries[lo].kind == kBrMass ? 16384 : pl.jobs.size();
                for (hi = lo + 1; hi < pl.jobs.size() && hi - lo < most && pl.entries[hi].key == pl.entries[lo].key; ++hi) {}
                launch(pl.entries[lo].kind, pl.entries[lo].round, job_table + lo, uint32_t(hi - lo), &pl.jobs[lo]);
            }
        }
        if (err == hipSuccess) err = hipMemcpyAsync(root_host, pl.root, side[p].n * sizeof(double), hipMemcpyDeviceToHost, t->stream);
        if (cfr && gadget == p && gadget_kind == RS_GADGET_RESOLVE) {   // the resolver's sweep: the TERMINATE leaf's row comes back beside the root's
            gadget_term.resize(side[p].n);
            if (err == hipSuccess) err = hipMemcpyAsync(gadget_term.data(), d_g_row[p], side[p].n * sizeof(double), hipMemcpyDeviceToHost, t->stream);
        }
        if (cfr && gadget >= 0 && gadget_kind == RS_GADGET_MAXMARGIN && err == hipSuccess)   // max-margin: U (the opponent's sweep) and the sum of rho * alt (the resolver's)
            err = hipMemcpyAsync(g_out, d_g_out, sizeof(g_out), hipMemcpyDeviceToHost, t->stream);
        const hipError_t done = hipStreamSynchronize(t->stream);   // the plan is freed on return and the next pass overwrites the job table: after an error too, nothing queued may still touch them
        if (err == hipSuccess) err = done;
        return err == hipSuccess ? RS_OK : hip_fail(err, ws_levels ? "rs_best_response (level plan)" : "rs_best_response");
    }
    std::vector<double> gadget_term;   // the TERMINATE leaf's row of the last resolver's sweep
    int traverse(int traverser, std::vector<double> &root, double *total);
};

// run-outs of an initial board in the enumeration order of the lanes: the first new card most significant, cards ascending among those still in the deck
static size_t enumerate_runouts(const uint8_t *board0, int n_board0, std::vector<uint8_t> *out) {
    uint8_t deck[52];
    int D = 0;
    for (int c = 0; c < 52; ++c) {
        bool used = false;
        for (int i = 0; i < n_board0; ++i) used = used || board0[i] == c;
        if (!used) deck[D++] = uint8_t(c);
    }
    const int K = 5 - n_board0;
    size_t nb = 0;
    auto emit = [&](int c3, int c4) {
        if (out) {
            uint8_t row[5];
            for (int k = 0; k < n_board0; ++k) row[k] = board0[k];
            if (K == 2) row[3] = uint8_t(c3);
            if (K >= 1) row[4] = uint8_t(c4);
            out->insert(out->end(), row, row + 5);
        }
        ++nb;
    };
    if (K == 0) emit(0, 0);
    else if (K == 1)
        for (int i = 0; i < D; ++i) emit(0, deck[i]);
    else
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                if (j != i) emit(deck[i], deck[j]);
    return nb;
}

}  // namespace rs

extern "C" {

size_t rs_br_runouts(const uint8_t *board0, int n_board0, uint8_t *out_cards) {
    if (!board0 || n_board0 < 3 || n_board0 > 5) return 0;
    std::vector<uint8_t> cards;
    const size_t nb = enumerate_runouts(board0, n_board0, out_cards ? &cards : nullptr);
    if (out_cards) std::memcpy(out_cards, cards.data(), cards.size());
    return nb;
}

// host only; the one place the raked payoffs are worked out (build_plan calls it for every terminal of a raked run)
int rs_rake_payoffs(const rs_tree *tree, int node, const rs_rake *rake, int player, double out[3]) {
    if (!tree || !out) return rs::fail(RS_ERR_INVALID, "rs_rake_payoffs: NULL argument");
    if (player != 0 && player != 1) return rs::fail(RS_ERR_INVALID, "rs_rake_payoffs: player is 0 or 1");
    if (node < 0 || size_t(node) >= tree->nodes.size()) return rs::fail(RS_ERR_INVALID, "rs_rake_payoffs: node id " + std::to_string(node) + " is out of range");
    const rs_tree_node &n = tree->nodes[size_t(node)];
    if (n.kind != RS_NODE_TERMINAL) return rs::fail(RS_ERR_INVALID, "rs_rake_payoffs: node " + std::to_string(node) + " is not a terminal");
    if (int rc = rs::br_check_rake(rake)) return rc;
    const double pot = double(float(n.value));
    const double r = rake ? std::min(rake->cap, rake->rate * pot) : 0.0;
    if (n.ttype == RS_TERM_UNCONTESTED) out[0] = out[1] = out[2] = player == int(n.last_to_act) ? -pot : pot - r;
    else out[0] = pot - r, out[1] = r > 0.0 ? -0.5 * r : 0.0, out[2] = -pot;
    return RS_OK;
}

}  // extern "C"

namespace rs {

// Everything of a best-response pass that depends on the GAME only (tree shape, ranges, board, cluster ids) and not on the table's contents: lane scores and masks, the lanes of
// every info set in ascending order, the rank-order index of the showdowns, the walk's buffers.  A caller that asks again for the same game (the trainer's exploitability
// ticks) keeps the object and pays for the walk alone.
// The run-outs fall into components (two run-outs that hold lanes of one info set belong together); where the largest is small, components are packed into groups of
// `cap` run-outs and the round's own nodes go to k_br_own_grouped_jobs.  Random bucket files tie every run-out to every other: one component, no groups.
static void build_groups(BrRun &run, BrSide &s, int r, size_t NB, size_t H, const std::vector<uint32_t> &start, const std::vector<uint32_t> &order) {
    const uint32_t NC = s.n_clusters[r];
    if (H == 0 || H > size_t(kBrGroupPerThread) * kBrGroupBlock) return;
    std::vector<uint32_t> parent(NB);
    for (size_t b = 0; b < NB; ++b) parent[b] = uint32_t(b);
    auto find = [&](uint32_t b) {
        while (parent[b] != b) b = parent[b] = parent[parent[b]];
        return b;
    };
    for (uint32_t c = 0; c < NC; ++c) {
        const uint32_t lo = start[c], hi = start[size_t(c) + 1];
        if (lo == hi) continue;
        uint32_t b0 = find(uint32_t(order[lo] / H));
        for (uint32_t i = lo + 1; i < hi; ++i) {
            const uint32_t b = find(uint32_t(order[i] / H));
            if (b == b0) continue;
            if (b < b0) parent[b0] = b, b0 = b;
            else parent[b] = b0;
        }
    }
    std::vector<uint32_t> size(NB, 0);
    uint32_t largest = 0;
    for (size_t b = 0; b < NB; ++b) largest = std::max(largest, ++size[find(uint32_t(b))]);
    const uint32_t cap_max = uint32_t(size_t(kBrGroupPerThread) * kBrGroupBlock / H);
    if (largest > cap_max) return;
    const uint32_t cap = std::min(cap_max, std::max<uint32_t>(largest, std::max<uint32_t>(1, uint32_t(kBrGroupLanes / H))));
    // components in the order of their smallest cluster id, packed greedily: neighbours in that order hold neighbouring info sets -- the same 64-byte lines of the
    // strategy-sum rows (a lossless abstraction numbers its clusters hand by hand, then by the larger and the smaller of the two cards to come) -- and the reach kernel hands
    // neighbouring groups to one XCD
    std::vector<uint32_t> comp_order;
    {
        std::vector<char> seen(NB, 0);
        for (uint32_t c = 0; c < NC; ++c) {
            if (start[c] == start[size_t(c) + 1]) continue;
            const uint32_t root = find(uint32_t(order[start[c]] / H));
            if (!seen[root]) seen[root] = 1, comp_order.push_back(root);
        }
        for (size_t b = 0; b < NB; ++b)   // run-outs without a single info set (no hand fits): on their own, last
            if (find(uint32_t(b)) == b && !seen[b]) comp_order.push_back(uint32_t(b));
    }
    std::vector<uint32_t> group_of(NB, 0), slot_of(NB, 0), group_root(NB, 0xffffffffu);
    std::vector<uint32_t> runouts;
    uint32_t n_groups = 0, used = cap;
    for (uint32_t root : comp_order) {
        if (used + size[root] > cap) {
            ++n_groups;
            used = 0;
            runouts.resize(size_t(n_groups) * cap, 0xffffffffu);
        }
        group_root[root] = n_groups - 1;
        used += size[root];
    }
    for (size_t b = 0; b < NB; ++b) {   // members take their group's slots in ascending order
        const uint32_t g = group_root[find(uint32_t(b))];
        group_of[b] = g;
        uint32_t slot = 0;
        while (runouts[size_t(g) * cap + slot] != 0xffffffffu) ++slot;
        runouts[size_t(g) * cap + slot] = uint32_t(b);
        slot_of[b] = slot;
    }
    std::vector<uint32_t> cstart(size_t(n_groups) + 1, 0);
    for (uint32_t c = 0; c < NC; ++c)
        if (start[c] != start[size_t(c) + 1]) cstart[size_t(group_of[order[start[c]] / H]) + 1]++;
    uint32_t max_sets = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        max_sets = std::max(max_sets, cstart[size_t(g) + 1]);
        cstart[size_t(g) + 1] += cstart[g];
    }
    const size_t lds = (size_t(cap) * H + max_sets) * sizeof(double) + size_t(max_sets) * sizeof(uint32_t);
    if (lds > size_t(150) << 10) return;
    const uint32_t n_sets = cstart[n_groups];
    std::vector<uint32_t> lstart(size_t(n_sets) + 1, 0), at(cstart.begin(), cstart.end() - 1), set_of(NC, 0xffffffffu);
    for (uint32_t c = 0; c < NC; ++c)   // ascending cluster id within a group
        if (start[c] != start[size_t(c) + 1]) {
            const uint32_t k = at[group_of[order[start[c]] / H]]++;
            set_of[c] = k;
            lstart[size_t(k) + 1] = start[size_t(c) + 1] - start[c];
        }
    for (uint32_t k = 0; k < n_sets; ++k) lstart[size_t(k) + 1] += lstart[k];
    std::vector<uint16_t> llane(lstart[n_sets]), lane_set(size_t(n_groups) * cap * H, uint16_t(0xffff));
    for (uint32_t c = 0; c < NC; ++c) {
        if (set_of[c] == 0xffffffffu) continue;
        uint32_t o = lstart[set_of[c]];
        const uint32_t grp = group_of[order[start[c]] / H];
        for (uint32_t i = start[c]; i < start[size_t(c) + 1]; ++i) {
            const uint32_t b = uint32_t(order[i] / H), local = uint32_t(slot_of[b] * H + (order[i] - b * H));
            llane[o++] = uint16_t(local);
            lane_set[size_t(grp) * cap * H + local] = uint16_t(set_of[c] - cstart[grp]);
        }
    }
    BrGroups &g = s.groups[r];
    g.runouts = run.upload(runouts);
    g.cstart = run.upload(cstart);
    g.lstart = run.upload(lstart);
    g.llane = run.upload(llane);
    g.lane_set = run.upload(lane_set);
    {
        std::vector<uint32_t> set_cluster(n_sets, 0);
        for (uint32_t c = 0; c < NC; ++c)
            if (set_of[c] != 0xffffffffu) set_cluster[set_of[c]] = c;
        g.set_cluster = run.upload(set_cluster);
    }
    g.n_groups = n_groups;
    g.cap = cap;
    g.n_hands = uint32_t(H);
    g.max_sets = max_sets;
    s.group_lds[r] = lds;
    s.grouped[r] = n_groups > 0;
}

// Own nodes by columns (k_br_own_cols_jobs): the info sets ordered by their first lane, their lane lists transposed.  Taken where neighbours in that order mostly hold
// neighbouring lanes (a lossless abstraction: the same cards under the next hand) and the lists are of a length a single thread walks (32 .. 2 048 lanes per info set).
static void build_columns(BrRun &run, BrSide &s, int r, const std::vector<uint32_t> &start, const std::vector<uint32_t> &order) {
    const uint32_t NC = s.n_clusters[r];
    std::vector<uint32_t> perm;
    uint32_t kmax = 0;
    for (uint32_t c = 0; c < NC; ++c)
        if (start[c] != start[size_t(c) + 1]) {
            perm.push_back(c);
            kmax = std::max(kmax, start[size_t(c) + 1] - start[c]);
        }
    if (perm.size() < 2 || kmax > 2048 || size_t(kmax) * perm.size() > (size_t(1) << 27)) return;
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return order[start[a]] < order[start[b]]; });
    size_t side_by_side = 0;
    for (size_t i = 0; i + 1 < perm.size(); ++i) side_by_side += order[start[perm[i + 1]]] == order[start[perm[i]]] + 1;
    if (side_by_side * 2 < perm.size()) return;
    const size_t n_sets = perm.size();
    std::vector<uint32_t> tord(size_t(kmax) * n_sets, 0xffffffffu);
    for (size_t i = 0; i < n_sets; ++i)
        for (uint32_t k = 0, lo = start[perm[i]], n = start[size_t(perm[i]) + 1] - lo; k < n; ++k) tord[size_t(k) * n_sets + i] = order[lo + k];
    s.d_tord[r] = run.upload(tord);
    s.d_perm[r] = run.upload(perm);
    s.n_sets[r] = uint32_t(n_sets);
    s.kmax[r] = kmax;
}

// The two lane rows of a game with weighted ranges (rs_range_weights; the header states both distributions).  Z0(b) on the host, Z1(b, h0) per lane on the device into
// player 0's row, which k_br_weighted_lanes then turns into the lane factor in place; the joint distribution's Z is the host's sum, ascending from 0.0, over the row
// copied back in between.  Failures land in run.err, like every other step of br_prepare.
static void br_weighted_rows(BrRun &run, const rs_range_weights &weights, const std::vector<uint64_t> &mask0, const std::vector<uint64_t> &bmask, double pb) {
    BrSide &s0 = run.side[0], &s1 = run.side[1];
    hipStream_t stream = run.t->stream;
    const size_t NB = run.NB, n0 = s0.n_hands, n1 = s1.n_hands;
    std::vector<double> w0(n0, 1.0), w1(n1, 1.0);
    if (weights.w[0]) w0.assign(weights.w[0], weights.w[0] + n0);
    if (weights.w[1]) w1.assign(weights.w[1], weights.w[1] + n1);
    const bool joint = weights.deal == RS_DEAL_JOINT;
    double *d_w0 = run.upload(w0), *d_w1 = run.upload(w1), *d_z0 = nullptr;
    if (!joint) {
        std::vector<double> z0(NB, 0.0);
        for (size_t b = 0; b < NB; ++b)
            for (size_t h = 0; h < n0; ++h)
                if ((mask0[h] & bmask[b]) == 0) z0[b] += w0[h];
        d_z0 = run.upload(z0);
    }
    double *d_row0 = run.dalloc<double>(s0.n), *d_row1 = run.dalloc<double>(s1.n);
    if (run.err != hipSuccess) return;
    hipLaunchKernelGGL(k_br_weighted_z1, dim3(grid1(s0.n_hands), uint32_t(NB)), dim3(kBrBlock), n1 * (sizeof(double) + sizeof(uint64_t)), stream, s0.d_mask, s0.n_hands,
                       s1.d_mask, d_w1, s1.n_hands, run.d_bmask, d_row0);
    if ((run.err = hipGetLastError()) != hipSuccess) return;
    double scale = pb;
    if (joint) {
        std::vector<double> z1(s0.n);
        run.err = hipMemcpyAsync(z1.data(), d_row0, z1.size() * sizeof(double), hipMemcpyDeviceToHost, stream);
        if (run.err == hipSuccess) run.err = hipStreamSynchronize(stream);
        if (run.err != hipSuccess) return;
        scale = 0.0;
        for (size_t b = 0; b < NB; ++b)
            for (size_t h = 0; h < n0; ++h)
                if ((mask0[h] & bmask[b]) == 0) scale += w0[h] * z1[b * n0 + h];
    }
    hipLaunchKernelGGL(k_br_weighted_lanes, dim3(grid1(s0.n)), dim3(kBrBlock), 0, stream, d_w0, s0.n_hands, d_z0, uint32_t(NB), scale, d_row0);
    if ((run.err = hipGetLastError()) != hipSuccess) return;
    hipLaunchKernelGGL(k_br_tile_weights, dim3(grid1(s1.n)), dim3(kBrBlock), 0, stream, d_w1, s1.n_hands, uint32_t(NB), d_row1);
    run.err = hipGetLastError();
    s0.d_init_q = s0.d_pw = d_row0;
    s1.d_init_q = s1.d_pw = d_row1;
}

// rs_range_weights as the header states them; NULL = no weights.  Touches nothing: the weighted entry points call it before anything is allocated or written
int br_check_weights(const rs_range_weights *weights, size_t n_hands_p0, size_t n_hands_p1) {
    if (!weights) return RS_OK;
    if (weights->deal != RS_DEAL_SEQUENTIAL && weights->deal != RS_DEAL_JOINT) return fail(RS_ERR_INVALID, "rs_range_weights: deal is RS_DEAL_SEQUENTIAL or RS_DEAL_JOINT");
    if (weights->reserved != 0) return fail(RS_ERR_INVALID, "rs_range_weights: reserved must be 0");
    const size_t n_hands[2] = {n_hands_p0, n_hands_p1};
    for (int p = 0; p < 2; ++p) {
        if (!weights->w[p]) continue;
        if (n_hands[p] == 0 || n_hands[p] > 1326) return fail(RS_ERR_INVALID, "rs_best_response: 1..1326 hands per range");
        double sum = 0.0;
        for (size_t h = 0; h < n_hands[p]; ++h) {
            const double w = weights->w[p][h];
            if (!(w > 0.0) || !std::isfinite(w))
                return fail(RS_ERR_INVALID, "rs_range_weights: weight " + std::to_string(h) + " of player " + std::to_string(p) +
                                                " is not finite and > 0 (a hand that is not in the range is left out of the list)");
            sum += w;
        }
        if (!std::isfinite(sum)) return fail(RS_ERR_INVALID, "rs_range_weights: the weights of player " + std::to_string(p) + " do not add up to a finite number");
    }
    return RS_OK;
}

// ---- node locks: the shape of a lock and the refusals, host only -----------------------------------------------------------------------------------------------------
// the doubles of `node`'s lock, A * (prefixes of its round) * n_hands of the acting player; 0 and rs_last_error on bad arguments.  *prefixes (may be NULL): the middle factor
static size_t br_lock_layout(const rs_tree *tree, int n_board0, size_t n_hands, int node, size_t *prefixes) {
    const auto bad = [](const std::string &why) {
        (void)fail(RS_ERR_INVALID, "rs_node_locks: " + why);
        return size_t(0);
    };
    if (!tree) return bad("NULL argument");
    if (n_board0 < 3 || n_board0 > 5) return bad("the initial board has 3, 4 or 5 cards");
    if (n_hands == 0 || n_hands > 1326) return bad("1..1326 hands in the acting player's range");
    if (node < 0 || size_t(node) >= tree->nodes.size()) return bad("node id " + std::to_string(node) + " is out of range");
    const rs_tree_node &n = tree->nodes[size_t(node)];
    if (n.kind != RS_NODE_ACTION) return bad("node " + std::to_string(node) + " is not an action node");
    const int K = 5 - n_board0, D = 52 - n_board0;
    if (n.n_children < 1 || n.n_children > RS_MAX_ACTIONS || int(n.round_idx) > K || n.player > 1) return bad("node " + std::to_string(node) + " has no place in a game from this board");
    size_t f = 1;
    for (int i = 0; i < int(n.round_idx); ++i) f *= size_t(D - i);
    if (prefixes) *prefixes = f;
    return size_t(n.n_children) * f * n_hands;
}

int br_check_locks(const rs_node_locks *locks, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                   size_t n_hands_p1) {
    if (!locks || locks->n == 0) return RS_OK;
    if (!tree || !board0 || !hands_p0 || !hands_p1 || !locks->nodes || !locks->sigma) return fail(RS_ERR_INVALID, "rs_node_locks: NULL argument");
    if (n_board0 < 3 || n_board0 > 5) return fail(RS_ERR_INVALID, "rs_node_locks: the initial board has 3, 4 or 5 cards");
    const uint8_t *hands[2] = {hands_p0, hands_p1};
    const size_t n_hands[2] = {n_hands_p0, n_hands_p1};
    std::vector<uint8_t> cards;   // the run-outs: prefix f of round r is the first r new cards of run-out f * (run-outs under a prefix of round r)
    const size_t NB = enumerate_runouts(board0, n_board0, &cards);
    std::vector<char> seen(tree->nodes.size(), 0);
    for (uint32_t k = 0; k < locks->n; ++k) {
        const int32_t id = locks->nodes[k];
        size_t F = 0;
        const size_t actor_hands = id >= 0 && size_t(id) < tree->nodes.size() ? n_hands[tree->nodes[size_t(id)].player & 1] : 1;
        const size_t total = br_lock_layout(tree, n_board0, actor_hands, id, &F);
        if (!total) return RS_ERR_INVALID;
        if (seen[size_t(id)]) return fail(RS_ERR_INVALID, "rs_node_locks: node " + std::to_string(id) + " is locked twice");
        seen[size_t(id)] = 1;
        const double *row = locks->sigma[k];
        if (!row) return fail(RS_ERR_INVALID, "rs_node_locks: the row of node " + std::to_string(id) + " is NULL");
        const rs_tree_node &n = tree->nodes[size_t(id)];
        const size_t H = actor_hands, A = size_t(n.n_children), pp = NB / F;
        for (size_t i = 0; i < total; ++i)
            if (!std::isfinite(row[i]) || row[i] < 0.0)
                return fail(RS_ERR_INVALID, "rs_node_locks: entry " + std::to_string(i) + " of node " + std::to_string(id) + " is not finite and >= 0");
        for (size_t f = 0; f < F; ++f) {
            uint64_t pm = 0;   // the prefix's new cards
            for (int i = 0; i < int(n.round_idx); ++i) pm |= 1ull << cards[f * pp * 5 + size_t(n_board0 + i)];
            for (size_t h = 0; h < H; ++h) {
                const uint8_t c0 = hands[n.player][2 * h], c1 = hands[n.player][2 * h + 1];
                if (c0 >= 52 || c1 >= 52) return fail(RS_ERR_INVALID, "rs_best_response: bad hole cards in a range");
                if (pm & (1ull << c0 | 1ull << c1)) continue;   // the pair shares a card: no deal, not sum-checked, never used
                double sum = 0.0;
                for (size_t a = 0; a < A; ++a) sum += row[(a * F + f) * H + h];
                if (!(std::fabs(sum - 1.0) <= 1e-9))
                    return fail(RS_ERR_INVALID, "rs_node_locks: the strategy of node " + std::to_string(id) + " at prefix " + std::to_string(f) + ", hand " + std::to_string(h) +
                                                    " sums to " + std::to_string(sum) + ", not to 1");
            }
        }
    }
    return RS_OK;
}

// rs_rake as the header states it; NULL = no rake.  Touches nothing: the raked entry points call it before anything is allocated or the table is settled
int br_check_rake(const rs_rake *rake) {
    if (!rake) return RS_OK;
    if (!std::isfinite(rake->rate) || rake->rate < 0.0 || rake->rate > 1.0) return fail(RS_ERR_INVALID, "rs_rake: rate is finite and in [0, 1]");
    if (std::isnan(rake->cap) || rake->cap < 0.0) return fail(RS_ERR_INVALID, "rs_rake: cap is >= 0 (+inf = uncapped)");
    if (rake->reserved[0] != 0 || rake->reserved[1] != 0) return fail(RS_ERR_INVALID, "rs_rake: reserved must be 0");
    return RS_OK;
}

int br_prepare(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
               size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, bool sorted, const rs_range_weights *weights, BrRun **prepared,
               const rs_node_locks *locks /* checked by the caller: br_check_locks */) {
    if (!t || !tree || !board0 || !hands_p0 || !hands_p1 || !cluster || !prepared) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    *prepared = nullptr;
    if (int rc = br_check_weights(weights, n_hands_p0, n_hands_p1)) return rc;
    if (tree->nodes.empty()) return fail(RS_ERR_INVALID, "rs_best_response: empty tree");
    if (n_board0 < 3 || n_board0 > 5) return fail(RS_ERR_INVALID, "rs_best_response: the initial board has 3, 4 or 5 cards (state.rs:59-64)");
    const int K = 5 - n_board0, D = 52 - n_board0;
    if (n_rounds < 1 || n_rounds > K + 1 || n_rounds > RS_MAX_ROUNDS) return fail(RS_ERR_INVALID, "rs_best_response: 1 .. (6 - board cards) betting rounds");
    if (n_hands_p0 == 0 || n_hands_p1 == 0 || n_hands_p0 > 1326 || n_hands_p1 > 1326) return fail(RS_ERR_INVALID, "rs_best_response: 1..1326 hands per range");
    if (int rc = check_tree_against_table(t, tree, "rs_best_response")) return rc;
    uint32_t n_clusters[RS_MAX_ROUNDS][2] = {{0, 0}, {0, 0}, {0, 0}};
    for (const rs_tree_node &n : tree->nodes) {
        if (n.kind != RS_NODE_ACTION) continue;
        const rs_node_desc &nd = t->nodes[size_t(n.index)];
        if (n.round_idx >= n_rounds) return fail(RS_ERR_INVALID, "rs_best_response: the tree has more betting rounds than n_rounds");
        if (nd.n_boards != 1 || t->tiled(n.index)) return fail(RS_ERR_UNSUPPORTED, "rs_best_response: tables of the reference's shape [action node][cluster] (n_boards = 1)");
        if (n.player > 1) return fail(RS_ERR_INVALID, "rs_best_response: two players");
        uint32_t &nc = n_clusters[n.round_idx][n.player];
        if (nc && nc != nd.n_clusters) return fail(RS_ERR_INVALID, "rs_best_response: a player's nodes of one round differ in cluster count");
        nc = nd.n_clusters;
    }
    uint64_t board_mask = 0;
    for (int i = 0; i < n_board0; ++i) {
        if (board0[i] >= 52 || (board_mask >> board0[i] & 1)) return fail(RS_ERR_INVALID, "rs_best_response: the board is distinct cards below 52");
        board_mask |= 1ull << board0[i];
    }
    const uint8_t *hands[2] = {hands_p0, hands_p1};
    const size_t n_hands[2] = {n_hands_p0, n_hands_p1};
    std::vector<uint64_t> mask[2];
    for (int p = 0; p < 2; ++p) {
        mask[p].resize(n_hands[p]);
        for (size_t h = 0; h < n_hands[p]; ++h) {
            const uint8_t a = hands[p][2 * h], b = hands[p][2 * h + 1];
            if (a >= 52 || b >= 52 || a == b) return fail(RS_ERR_INVALID, "rs_best_response: bad hole cards in a range");
            mask[p][h] = 1ull << a | 1ull << b;
            if (mask[p][h] & board_mask) return fail(RS_ERR_INVALID, "rs_best_response: a range combo uses a board card");
        }
    }
    if (sorted)   // the rank-order index lists the opponent's hands by card (at most kBrCardHolders per card) and knows ONE opponent hand per card pair (`same`)
        for (int p = 0; p < 2; ++p) {
            std::vector<uint64_t> m(mask[p]);
            std::sort(m.begin(), m.end());
            if (std::adjacent_find(m.begin(), m.end()) != m.end())
                return fail(RS_ERR_INVALID, "rs_best_response: RS_BR_SORTED takes ranges of distinct combos (a combo occurs twice in player " + std::to_string(p) + "'s range)");
        }
    std::vector<uint8_t> cards;
    const size_t NB = enumerate_runouts(board0, n_board0, &cards);
    if (NB * std::max(n_hands[0], n_hands[1]) >= (size_t(1) << 31)) return fail(RS_ERR_UNSUPPORTED, "rs_best_response: too many lanes");
    std::vector<uint64_t> bmask(NB, 0);
    std::vector<uint32_t> cnt0(NB, 0);
    for (size_t b = 0; b < NB; ++b) {
        for (int i = n_board0; i < 5; ++i) bmask[b] |= 1ull << cards[b * 5 + size_t(i)];
        for (size_t h = 0; h < n_hands[0]; ++h) cnt0[b] += (mask[0][h] & bmask[b]) == 0;
    }
    size_t per_prefix[RS_MAX_ROUNDS] = {1, 1, 1};
    for (int r = 0; r < n_rounds; ++r) {   // completions left after r new cards
        size_t left = 1;
        for (int i = r; i < K; ++i) left *= size_t(D - i);
        per_prefix[r] = left;
    }
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    std::unique_ptr<BrRun> owner(new BrRun);
    BrRun &run = *owner;
    run.t = t;
    run.tree = tree;
    run.sorted = sorted;
    run.NB = uint32_t(NB);
    run.n_board0 = n_board0;
    for (int r = 0; r < RS_MAX_ROUNDS; ++r) run.per_prefix[r] = uint32_t(per_prefix[r]);
    run.d_bmask = run.upload(bmask);
    uint8_t *d_boards = run.upload(cards);
    uint32_t *d_cnt0 = weights ? nullptr : run.upload(cnt0);   // (weighted ranges: Z0 takes its place, br_weighted_rows)
    for (int p = 0; p < 2; ++p) {
        BrSide &s = run.side[p];
        s.n_hands = uint32_t(n_hands[p]);
        s.n = uint32_t(NB * n_hands[p]);
        s.n_pad = uint32_t(round_up(size_t(s.n), 64));
        std::vector<uint8_t> hv(hands[p], hands[p] + 2 * n_hands[p]);
        uint8_t *d_hands = run.upload(hv);
        s.d_hands = d_hands;
        s.d_mask = run.upload(mask[p]);
        s.d_score = run.dalloc<uint32_t>(s.n);
        if (run.err == hipSuccess) {
            hipLaunchKernelGGL(k_lane_scores, dim3(grid1(s.n)), dim3(kBrBlock), 0, t->stream, d_hands, s.n_hands, d_boards, uint32_t(n_board0), uint32_t(NB), s.d_score);
            run.err = hipGetLastError();
        }
        for (int r = 0; r < n_rounds; ++r) {
            const uint32_t *src = cluster[size_t(r) * 2 + size_t(p)];
            s.n_clusters[r] = n_clusters[r][p];
            if (!s.n_clusters[r]) continue;   // the player has no node in this round
            if (!src) return fail(RS_ERR_INVALID, "rs_best_response: no cluster ids for round " + std::to_string(r) + " player " + std::to_string(p));
            // lane-level ids and, per info set, its lanes in ascending order.  A blocked lane (its hand uses a card of the run-out: no such deal) belongs to no
            // info set: it is listed in an extra segment after the last cluster (k_br_own_jobs writes its 0) and looks up cluster 0 where an id is needed but not used
            const uint32_t NC = s.n_clusters[r];
            std::vector<uint32_t> cv(s.n), seg(s.n), start(size_t(NC) + 2, 0), order(s.n);
            for (size_t b = 0; b < NB; ++b)
                for (size_t h = 0; h < n_hands[p]; ++h) {
                    uint32_t k = src[(b / per_prefix[r]) * n_hands[p] + h];
                    const bool blocked = (mask[p][h] & bmask[b]) != 0;
                    if (!blocked && k >= NC)
                        return fail(RS_ERR_OOB, "rs_best_response: cluster id " + std::to_string(k) + " of player " + std::to_string(p) + " is outside the table");
                    cv[b * n_hands[p] + h] = blocked ? 0u : k;
                    seg[b * n_hands[p] + h] = blocked ? NC : k;
                }
            for (uint32_t k : seg) start[size_t(k) + 1]++;
            for (size_t c = 0; c <= NC; ++c) start[c + 1] += start[c];
            {
                std::vector<uint32_t> fill(start.begin(), start.end() - 1);
                for (size_t l = 0; l < seg.size(); ++l) order[fill[seg[l]]++] = uint32_t(l);
            }
            s.d_cid[r] = run.upload(cv);
            s.d_start[r] = run.upload(start);
            s.d_order[r] = run.upload(order);
            if (size_t(s.n) < size_t(NC) * 32) build_groups(run, s, r, NB, n_hands[p], start, order);
            else build_columns(run, s, r, start, order);   // (what neither takes goes a thread per info set, or a wave where the info sets hold many lanes)
        }
    }
    if (sorted)   // the node-independent half of the rank-order showdowns: once per call
        for (int p = 0; p < 2; ++p) {
            BrSide &me = run.side[p], &op = run.side[1 - p];
            BrIndex &ix = me.index;
            ix.ord = run.dalloc<uint16_t>(NB * op.n_hands);
            ix.nv = run.dalloc<uint16_t>(NB);
            ix.cl = run.dalloc<uint16_t>(NB * 52 * kBrCardHolders);
            ix.cc = run.dalloc<uint8_t>(NB * 52);
            ix.nl = run.dalloc<uint16_t>(NB * me.n_hands);
            ix.nle = run.dalloc<uint16_t>(NB * me.n_hands);
            ix.kl = run.dalloc<uint8_t>(NB * me.n_hands * 2);
            ix.kle = run.dalloc<uint8_t>(NB * me.n_hands * 2);
            std::vector<int16_t> same(n_hands[p], -1);
            for (size_t h = 0; h < n_hands[p]; ++h)
                for (size_t g = 0; g < n_hands[1 - p]; ++g)
                    if (mask[p][h] == mask[1 - p][g]) same[h] = int16_t(g);
            ix.same = run.upload(same);
            if (run.err == hipSuccess) {
                hipLaunchKernelGGL(k_br_index, dim3(uint32_t(NB)), dim3(kBrBlock), 0, t->stream, me.d_hands, me.n_hands, me.d_mask, me.d_score, op.d_hands, op.n_hands, op.d_mask,
                                   op.d_score, run.d_bmask, ix);
                run.err = hipGetLastError();
            }
        }
    // the deal distribution of generate_hand (cfr.rs:100-143): the run-out uniform over ordered completions, player 0's combo uniform over the combos of its range
    // that avoid the full board, player 1's over those that avoid board and player 0: P = P(B) [disjoint] / (N0(B) N1(B, h0)); the whole weight rides on player 0's lane
    double pb = 1.0;
    for (int i = 0; i < K; ++i) pb /= double(D - i);
    if (weights) {
        br_weighted_rows(run, *weights, mask[0], bmask, pb);
    } else {
        double *d_w0 = run.dalloc<double>(run.side[0].n);
        if (run.err == hipSuccess) {
            hipLaunchKernelGGL(k_br_weights, dim3(grid1(run.side[0].n)), dim3(kBrBlock), 0, t->stream, run.side[0].d_mask, run.side[0].n_hands, run.side[1].d_mask,
                               run.side[1].n_hands, run.d_bmask, d_cnt0, uint32_t(NB), pb, d_w0);
            run.err = hipGetLastError();
        }
        std::vector<double> ones(run.side[1].n, 1.0);
        double *d_ones = run.upload(ones);
        run.side[0].d_init_q = run.side[0].d_pw = d_w0;
        run.side[1].d_init_q = run.side[1].d_pw = d_ones;
    }
    if (locks && locks->n) {   // the locks' rows: buffers of the prepared game (no slots of the walk's workspace), as given
        run.lock_of.assign(tree->nodes.size(), nullptr);
        for (uint32_t k = 0; k < locks->n; ++k) {
            const int32_t id = locks->nodes[k];
            const size_t total = br_lock_layout(tree, n_board0, n_hands[tree->nodes[size_t(id)].player], id, nullptr);
            run.lock_of[size_t(id)] = run.upload(std::vector<double>(locks->sigma[k], locks->sigma[k] + total));
        }
    }
    // the walk's buffers are allocated by every call (br_execute) and freed when it returns: a kept object holds what depends on the game only
    run.n_pad_max = std::max(run.side[0].n_pad, run.side[1].n_pad);
    run.fill_depths();
    if (run.err != hipSuccess) {
        (void)hipStreamSynchronize(t->stream);   // drain the stream before ~BrRun frees what queued kernels may still touch
        return hip_fail(run.err, "rs_best_response");
    }
    *prepared = owner.release();
    return RS_OK;
}

void br_free(BrRun *run) { delete run; }
size_t br_held_bytes(const BrRun *run) { return run ? run->dev_bytes : 0; }
void br_release_workspace(BrRun *run) {
    if (run) run->release_workspace();
}
int br_last_launches(const BrRun *run) { return run && run->last_level_plan ? run->last_launches : -1; }

static int br_check_mode(int mode /* without RS_BR_SORTED, RS_BR_REAL and RS_BR_CURRENT */, bool real) {
    if (mode != RS_BR_MAX && mode != RS_BR_AVERAGE)
        return fail(RS_ERR_INVALID, "rs_best_response: mode is RS_BR_MAX or RS_BR_AVERAGE (| RS_BR_SORTED, | RS_BR_CURRENT, RS_BR_MAX | RS_BR_REAL)");
    if (real && mode != RS_BR_MAX)
        return fail(RS_ERR_INVALID, "rs_best_response: RS_BR_REAL goes with RS_BR_MAX (the average strategy lives in the abstraction: RS_BR_AVERAGE | RS_BR_REAL means nothing)");
    return RS_OK;
}

// the walk's workspace: allocated by the first walk and kept with the object (see br_execute)
// A node report wants more than a best response's walk left behind -- the traverser's own reach rows, a mass row per requested node (level plan) or depth -- and trades a
// workspace that lacks them for a larger one; the walks that follow run on that (they take less of it).
static int br_ensure_workspace(BrRun &run, size_t mass_rows = 0) {
    const bool pi = run.takes_pi();
    if (run.ws && ((pi && !run.ws_pi) || (run.ws_levels && mass_rows > run.ws_mass_rows) || (!run.ws_levels && mass_rows && run.mass_level.empty()))) run.release_workspace();
    if (run.ws) return RS_OK;
    const size_t need = std::max(run.level_plan_bytes(0, pi, mass_rows), run.level_plan_bytes(1, pi, mass_rows));
    size_t free_b = 0, total_b = 0;
    const bool levels = !knobs_resolve(nullptr).br_depth_first && need <= kBrLevelPlanBytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= free_b / 2;
    (void)hipGetLastError();
    if (levels && run.ws.alloc(need / sizeof(double), &run.dev_bytes) == hipSuccess) {
        run.ws_levels = true;
        run.ws_pi = pi;
        run.ws_mass_rows = mass_rows;
    } else {
        int max_a = 1;
        for (const rs_tree_node &n : run.tree->nodes) max_a = std::max(max_a, n.n_children);
        const int depth = run.max_depth;   // only action nodes take a level of child buffers
        const size_t per = size_t(max_a) * run.n_pad_max, each = pi ? 3 : 2;   // reach and values; the traverser's own reach (full-width sweep, node report)
        const size_t mass = mass_rows ? size_t(depth) * run.n_pad_max : 0;            // a report's mass row per depth
        if (run.ws.alloc(each * size_t(depth) * per + run.n_pad_max + mass, &run.dev_bytes) != hipSuccess) return fail(RS_ERR_OOM, "rs_best_response: the walk's buffers");
        run.ws_levels = false;
        run.ws_pi = pi;
        for (int l = 0; l < depth; ++l) {
            run.q_level.push_back(run.ws + (each * size_t(l)) * per);
            run.v_level.push_back(run.ws + (each * size_t(l) + 1) * per);
            if (pi) run.pi_level.push_back(run.ws + (each * size_t(l) + 2) * per);
            if (mass) run.mass_level.push_back(run.ws + each * size_t(depth) * per + run.n_pad_max + size_t(l) * run.n_pad_max);
        }
        run.d_root = run.ws + each * size_t(depth) * per;
    }
    return RS_OK;
}

// One traverser's pass over the table as it stands, in the tree order of the workspace (allocated here by the first pass): its launches are added to last_launches (level
// plan), *total is the sum of the root's values, ascending like the oracle's.  root holds n_pad_max doubles.
int BrRun::traverse(int traverser, std::vector<double> &root, double *total) {
    if (int rc = br_ensure_workspace(*this, report_slot ? size_t(std::count_if(report_slot->begin(), report_slot->end(), [](int k) { return k >= 0; })) : 0)) return rc;
    last_level_plan = ws_levels;
    p = traverser;
    if (cfr) ++t->epoch;   // whatever happens below, rows may have been written
    if (int rc = run_traverser(root.data())) return rc;
    last_launches += ws_levels ? n_launches : 0;
    double sum = 0.0;
    for (uint32_t l = 0; l < side[p].n; ++l) sum += root[l];
    if (cfr && gadget == p && gadget_kind == RS_GADGET_RESOLVE) {   // plus the TERMINATE branch, summed like a root row
        double term = 0.0;
        for (uint32_t l = 0; l < side[p].n; ++l) term += gadget_term[l];
        sum += term;
    }
    if (cfr && gadget >= 0 && gadget_kind == RS_GADGET_MAXMARGIN) {   // max-margin: the rho-weighted margin under the current profile; the opponent's sweep is worth U
        if (gadget == p) sum += g_out[1];
        else sum = g_out[0], g_margin_ready = true;
    }
    *total = sum;
    return RS_OK;
}

void br_set_rake(BrRun *prepared, const rs_rake *rake) {
    prepared->raked = rake && rake->rate > 0.0 && rake->cap > 0.0;
    if (prepared->raked) prepared->rake = *rake;
}

// the walk: both traversers against the table as it stands
int br_execute(BrRun *prepared, int mode, double *out) {
    if (!prepared || !out) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    const bool real = (mode & RS_BR_REAL) != 0, current = (mode & RS_BR_CURRENT) != 0;
    mode &= ~(RS_BR_REAL | RS_BR_CURRENT);
    if (int rc = br_check_mode(mode, real)) return rc;
    BrRun &run = *prepared;
    if (run.cfr) return fail(RS_ERR_INVALID, "rs_best_response: the prepared game belongs to a full-width solver");
    rs_table *t = run.t;
    if (int rc = table_settle(t)) return rc;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    run.mode = mode;
    run.real = real;
    run.current = current;
    run.err = hipSuccess;
    // The level plan wants a buffer per tree edge (full 1 176-combo ranges from a flop on the 706-node tree: 59 GB, and an allocation of that size takes seconds; 200 combos: 10 GB)
    // and buys launches, not kernel time (4 300 -> 66 per call; at full ranges both orders spend 0.24-0.27 s in their kernels): it is taken while it fits kBrLevelPlanBytes and half
    // of the free memory, else the depth-first walk runs with its two buffers per tree depth.  The workspace is allocated by the first call and KEPT with the object
    // (br_workspace_bytes / br_release_workspace: a trainer holds one object per showdown mode).
    run.last_launches = 0;
    std::vector<double> root(run.n_pad_max);
    for (int p = 0; p < 2; ++p)
        if (int rc = run.traverse(p, root, &out[p])) return rc;
    return RS_OK;
}

// One traverser's walk with the root's mass row and the fold of both root rows behind the root's value job (rs_best_response_hands): value[h] and mass[h] of the
// traverser's hands, mass may be NULL.  Everything that can refuse has refused before the first launch, and the outputs are written after the last copy has come back.
int br_hands(BrRun *prepared, int mode, int traverser, double *value, double *mass) {
    if (!prepared || !value) return fail(RS_ERR_INVALID, "rs_best_response_hands: NULL argument");
    const bool real = (mode & RS_BR_REAL) != 0, current = (mode & RS_BR_CURRENT) != 0;
    mode &= ~(RS_BR_REAL | RS_BR_CURRENT);
    if (int rc = br_check_mode(mode, real)) return rc;
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_best_response_hands: traverser is 0 or 1");
    BrRun &run = *prepared;
    if (run.cfr) return fail(RS_ERR_INVALID, "rs_best_response_hands: the prepared game belongs to a full-width solver");
    rs_table *t = run.t;
    if (int rc = table_settle(t)) return rc;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    run.mode = mode;
    run.real = real;
    run.current = current;
    run.err = hipSuccess;
    const size_t n = run.side[traverser].n_hands;
    DevBuf<double> d_mass, d_out;
    RS_HIP(d_mass.alloc(run.side[traverser].n_pad), "rs_best_response_hands: the mass row");
    RS_HIP(d_out.alloc(2 * n), "rs_best_response_hands: the output buffer");
    run.d_hands_mass = d_mass;
    run.d_hands_out = d_out;
    run.last_launches = 0;
    std::vector<double> root(run.n_pad_max), host(2 * n);
    double total = 0.0;
    int rc = run.traverse(traverser, root, &total);   // synchronises: nothing queued touches the two buffers after it
    run.d_hands_mass = run.d_hands_out = nullptr;
    if (rc) return rc;
    RS_HIP(hipMemcpy(host.data(), d_out, 2 * n * sizeof(double), hipMemcpyDeviceToHost), "rs_best_response_hands: the copy back");
    std::copy(host.begin(), host.begin() + n, value);
    if (mass) std::copy(host.begin() + n, host.end(), mass);
    return RS_OK;
}

// ---- the node report on a prepared game ---------------------------------------------------------------------------------------------------------------------------
// the root reach of the traverser's own lanes: 1.0 (full-width sweep, node report)
static int br_root_reach(BrRun &run, const char *what) {
    for (int p = 0; p < 2; ++p)
        if (!run.d_pi0[p]) {
            const std::vector<double> ones(run.side[p].n, 1.0);
            run.d_pi0[p] = run.upload(ones);
            if (run.err != hipSuccess) return hip_fail(run.err, what);
        }
    return RS_OK;
}
// blocks of the requested nodes: offsets[k] doubles into the output, (A + 3) rows of [prefixes of the node's round][n_hands]; 0 and rs_last_error on bad arguments
static size_t br_report_layout(const rs_tree *tree, int n_board0, size_t n_hands, const int32_t *nodes, size_t n_nodes, uint64_t *offsets) {
    const auto bad = [](const std::string &why) {
        (void)fail(RS_ERR_INVALID, "rs_node_report: " + why);
        return size_t(0);
    };
    if (!tree || !nodes || n_nodes == 0) return bad("NULL argument or no nodes");
    if (n_board0 < 3 || n_board0 > 5) return bad("the initial board has 3, 4 or 5 cards");
    if (n_hands == 0 || n_hands > 1326) return bad("1..1326 hands in the traverser's range");
    const int K = 5 - n_board0, D = 52 - n_board0;
    std::vector<char> seen(tree->nodes.size(), 0);
    size_t total = 0;
    for (size_t k = 0; k < n_nodes; ++k) {
        const int32_t id = nodes[k];
        if (id < 0 || size_t(id) >= tree->nodes.size()) return bad("node id " + std::to_string(id) + " is out of range");
        const rs_tree_node &n = tree->nodes[size_t(id)];
        if (n.kind != RS_NODE_ACTION) return bad("node " + std::to_string(id) + " is not an action node");
        if (seen[size_t(id)]) return bad("node " + std::to_string(id) + " is asked for twice");
        seen[size_t(id)] = 1;
        if (n.n_children < 1 || n.n_children > RS_MAX_ACTIONS || int(n.round_idx) > K) return bad("node " + std::to_string(id) + " has no place in a game from this board");
        size_t prefixes = 1;
        for (int i = 0; i < int(n.round_idx); ++i) prefixes *= size_t(D - i);
        if (offsets) offsets[k] = uint64_t(total);
        total += size_t(n.n_children + 3) * prefixes * n_hands;
    }
    return total;
}

static int br_report_check_mode(int mode /* without RS_BR_SORTED */, int traverser) {
    if (mode != RS_BR_AVERAGE && mode != (RS_BR_AVERAGE | RS_BR_CURRENT))
        return fail(RS_ERR_INVALID, "rs_node_report: the report is of the strategy profile itself: mode is RS_BR_AVERAGE (| RS_BR_CURRENT, | RS_BR_SORTED)");
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_node_report: traverser is 0 or 1");
    return RS_OK;
}

// One traverser's RS_BR_AVERAGE walk with its own reach taken down beside q, the report jobs of the requested nodes behind their value jobs; the output buffer lives on
// the device for the call and comes back in one copy.  Everything that can refuse has refused before the first launch: a refused call leaves `out` alone.
int br_report(BrRun *prepared, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    if (!prepared || !out) return fail(RS_ERR_INVALID, "rs_node_report: NULL argument");
    if (int rc = br_report_check_mode(mode, traverser)) return rc;
    BrRun &run = *prepared;
    if (run.cfr) return fail(RS_ERR_INVALID, "rs_node_report: the prepared game belongs to a full-width solver");
    std::vector<uint64_t> offsets(n_nodes);
    const size_t total = br_report_layout(run.tree, run.n_board0, run.side[traverser].n_hands, nodes, n_nodes, offsets.data());
    if (!total) return RS_ERR_INVALID;
    if (out_doubles < total) return fail(RS_ERR_INVALID, "rs_node_report: the output buffer is too small (rs_node_report_size doubles)");
    std::vector<int> slot_of(run.tree->nodes.size(), -1);
    for (size_t k = 0; k < n_nodes; ++k) slot_of[size_t(nodes[k])] = int(k);
    rs_table *t = run.t;
    if (int rc = table_settle(t)) return rc;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    run.mode = RS_BR_AVERAGE;
    run.real = false;
    run.current = (mode & RS_BR_CURRENT) != 0;
    run.err = hipSuccess;
    if (int rc = br_root_reach(run, "rs_node_report: the root reach")) return rc;
    DevBuf<double> d_out;
    RS_HIP(d_out.alloc(total), "rs_node_report: the output buffer");
    run.report_slot = &slot_of;
    run.report_off = offsets.data();
    run.d_report = d_out;
    run.last_launches = 0;
    std::vector<double> root(run.n_pad_max);
    double value = 0.0;
    int rc = run.traverse(traverser, root, &value);   // synchronises: nothing queued touches d_out after it
    run.report_slot = nullptr;
    run.report_off = nullptr;
    run.d_report = nullptr;
    if (rc) return rc;
    RS_HIP(hipMemcpy(out, d_out, total * sizeof(double), hipMemcpyDeviceToHost), "rs_node_report: the copy back");
    return RS_OK;
}

// ---- the full-width sweep on a prepared game ---------------------------------------------------------------------------------------------------------------------
// One traverser's sweep over the table as it stands; *value = the sum of the root's values, ascending (the traverser's value per deal under the current profile).
// It WRITES the table: a training loop's working copy is settled first and kept shadow records are invalidated (rs_table.epoch), as every other writer does.
int br_cfr_mark(BrRun *prepared) {
    if (!prepared) return fail(RS_ERR_INVALID, "rs_range_cfr: NULL argument");
    if (prepared->ws) return fail(RS_ERR_INVALID, "rs_range_cfr: the prepared game has walked already");
    if (prepared->t->dtype != RS_F32)
        return fail(RS_ERR_UNSUPPORTED, "rs_range_cfr: RS_F32 tables only (the sums are per-deal probabilities times pots: no integer scale, and binary16 cells are out of scope)");
    prepared->cfr = true;
    return RS_OK;
}
static int br_mm_mass(BrRun &run);
int br_cfr_sweep(BrRun *prepared, int traverser, int rmplus, double *value) {
    if (!prepared || !prepared->cfr) return fail(RS_ERR_INVALID, "rs_range_cfr: NULL argument");
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_range_cfr_iterate: traverser is 0 or 1");
    BrRun &run = *prepared;
    rs_table *t = run.t;
    if (int rc = table_settle(t, true)) return rc;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    run.mode = RS_BR_AVERAGE;
    run.real = run.current = false;
    run.cfr_rmplus = rmplus ? 1 : 0;
    run.err = hipSuccess;
    if (int rc = br_root_reach(run, "rs_range_cfr: the root reach")) return rc;
    if (run.gadget >= 0 && run.gadget_kind == RS_GADGET_MAXMARGIN && !run.g_M_ready)   // the first sweep since arming, whichever traverser's
        if (int rc = br_mm_mass(run)) return rc;
    run.last_launches = 0;
    std::vector<double> root(run.n_pad_max);
    double total = 0.0;
    if (int rc = run.traverse(traverser, root, &total)) return rc;
    if (value) *value = total;
    return RS_OK;
}

// ---- the re-solving gadget on a full-width solver's prepared game ---------------------------------------------------------------------------------------------------
// Everything that can refuse has refused before anything is written: a refused call leaves the rows and the table alone.
int br_cfr_set_gadget(BrRun *prepared, int kind, int resolver, const double *alt) {
    if (!prepared || !prepared->cfr || !alt) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget: NULL argument");
    if (kind != RS_GADGET_RESOLVE && kind != RS_GADGET_MAXMARGIN) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget_kind: kind is RS_GADGET_RESOLVE or RS_GADGET_MAXMARGIN");
    if (resolver != 0 && resolver != 1) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget: resolver is 0 or 1");
    BrRun &run = *prepared;
    if (!run.lock_of.empty()) return fail(RS_ERR_UNSUPPORTED, "rs_range_cfr_set_gadget: the object was created with node locks (a gadget and locks on one object are out of scope)");
    if (run.raked) return fail(RS_ERR_UNSUPPORTED, "rs_range_cfr_set_gadget: the object was created with rake (the gadget's TERMINATE branch is a zero-sum construction)");
    const uint32_t n = run.side[1 - resolver].n_hands;
    for (uint32_t h = 0; h < n; ++h)
        if (!std::isfinite(alt[h])) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget: alt[" + std::to_string(h) + "] is not finite");
    rs_table *t = run.t;
    RS_HIP(hipSetDevice(t->device), "hipSetDevice");
    RS_HIP(hipStreamSynchronize(t->stream), "rs_range_cfr_set_gadget");
    run.err = hipSuccess;
    if (!run.d_g_alt) {   // first arming: the rows' buffers, kept with the object and sized for either player as the resolver
        const size_t most = std::max(run.side[0].n_hands, run.side[1].n_hands);
        double *a = run.dalloc<double>(most), *qf = run.dalloc<double>(run.n_pad_max), *qt = run.dalloc<double>(run.n_pad_max);
        double *row0 = run.dalloc<double>(run.side[0].n_pad), *row1 = run.dalloc<double>(run.side[1].n_pad);
        float *rg = run.dalloc<float>(2 * most), *ss = run.dalloc<float>(2 * most);
        if (run.err != hipSuccess) return hip_fail(run.err, "rs_range_cfr_set_gadget: the gadget's rows");
        run.d_g_alt = a, run.d_g_qf = qf, run.d_g_qt = qt, run.d_g_row[0] = row0, run.d_g_row[1] = row1, run.d_g_regret = rg, run.d_g_ssum = ss;
    }
    if (kind == RS_GADGET_MAXMARGIN && !run.d_g_M) {   // first max-margin arming: the per-hand rows, sized like alt
        const size_t most = std::max(run.side[0].n_hands, run.side[1].n_hands);
        double *f = run.dalloc<double>(most), *m = run.dalloc<double>(most), *sc = run.dalloc<double>(most), *mg = run.dalloc<double>(most), *o = run.dalloc<double>(2);
        if (run.err != hipSuccess) return hip_fail(run.err, "rs_range_cfr_set_gadget_kind: the max-margin rows");
        run.d_g_F = f, run.d_g_M = m, run.d_g_scale = sc, run.d_g_margin = mg, run.d_g_out = o;
    }
    RS_HIP(hipMemcpy(run.d_g_alt, alt, size_t(n) * sizeof(double), hipMemcpyHostToDevice), "rs_range_cfr_set_gadget: alt");
    RS_HIP(hipMemset(run.d_g_regret, 0, size_t(2) * n * sizeof(float)), "rs_range_cfr_set_gadget: the rows");
    RS_HIP(hipMemset(run.d_g_ssum, 0, size_t(2) * n * sizeof(float)), "rs_range_cfr_set_gadget: the rows");
    RS_HIP(hipDeviceSynchronize(), "rs_range_cfr_set_gadget");
    run.gadget = resolver;
    run.gadget_kind = kind;
    run.g_M_ready = run.g_margin_ready = false;
    return RS_OK;
}
// max-margin, in front of the first sweep since arming: M, which both sweeps read and which is a function of the prepared game alone -- the root's mass row on the
// opponent's lanes (the leaf kernels of the run's showdown mode on the resolver's initial reach: the kBrMass job of CFR-D's opponent sweep) and its fold, kept on the device.
static int br_mm_mass(BrRun &run) {
    if (int rc = br_ensure_workspace(run)) return rc;
    const int O = 1 - run.gadget;
    run.p = O;
    BrJob jm{};
    jm.q = run.side[run.gadget].d_init_q;
    jm.v = run.d_g_row[O];
    jm.uncontested = 1;
    jm.value = 1.0;
    if (run.job_table.bytes() < sizeof(BrJob)) run.err = run.job_table.alloc(1);
    if (run.err == hipSuccess) run.err = hipMemcpyAsync(run.job_table, &jm, sizeof(BrJob), hipMemcpyHostToDevice, run.t->stream);
    run.launch(kBrMass, 0, run.job_table, 1, &jm);
    const BrSide &me = run.side[O];
    if (run.err == hipSuccess) {
        hipLaunchKernelGGL(k_br_hands_fold, dim3(grid1(me.n_hands)), dim3(kBrBlock), 0, run.t->stream, me.d_mask, run.d_bmask, me.n_hands, run.NB, run.d_g_row[O], run.d_g_row[O],
                           run.d_g_F, run.d_g_M);
        run.err = hipGetLastError();
    }
    const hipError_t done = hipStreamSynchronize(run.t->stream);   // jm leaves scope
    if (run.err == hipSuccess) run.err = done;
    if (run.err != hipSuccess) return hip_fail(run.err, "rs_range_cfr: the max-margin gadget's mass row");
    run.g_M_ready = true;
    return RS_OK;
}
int br_cfr_gadget_margins(BrRun *prepared, double *out) {
    if (!prepared || !prepared->cfr || !out) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_margins: NULL argument");
    BrRun &run = *prepared;
    if (run.gadget < 0 || run.gadget_kind != RS_GADGET_MAXMARGIN) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_margins: the object has no max-margin gadget");
    if (!run.g_margin_ready) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_margins: no sweep of the opponent since the gadget was armed");
    RS_HIP(hipSetDevice(run.t->device), "hipSetDevice");
    RS_HIP(hipStreamSynchronize(run.t->stream), "rs_range_cfr_gadget_margins");
    RS_HIP(hipMemcpy(out, run.d_g_margin, size_t(run.side[1 - run.gadget].n_hands) * sizeof(double), hipMemcpyDeviceToHost), "rs_range_cfr_gadget_margins");
    return RS_OK;
}
int br_cfr_gadget_rows(BrRun *prepared, float *regrets, float *strategy_sum, const float *set_regrets, const float *set_strategy_sum, const char *fn) {
    if (!prepared || !prepared->cfr) return fail(RS_ERR_INVALID, std::string(fn) + ": NULL argument");
    BrRun &run = *prepared;
    if (run.gadget < 0) return fail(RS_ERR_INVALID, std::string(fn) + ": the object has no gadget (rs_range_cfr_set_gadget first)");
    const size_t bytes = size_t(2) * run.side[1 - run.gadget].n_hands * sizeof(float);
    RS_HIP(hipSetDevice(run.t->device), "hipSetDevice");
    RS_HIP(hipStreamSynchronize(run.t->stream), fn);
    if (regrets) RS_HIP(hipMemcpy(regrets, run.d_g_regret, bytes, hipMemcpyDeviceToHost), fn);
    if (strategy_sum) RS_HIP(hipMemcpy(strategy_sum, run.d_g_ssum, bytes, hipMemcpyDeviceToHost), fn);
    if (set_regrets) RS_HIP(hipMemcpy(run.d_g_regret, set_regrets, bytes, hipMemcpyHostToDevice), fn);
    if (set_strategy_sum) RS_HIP(hipMemcpy(run.d_g_ssum, set_strategy_sum, bytes, hipMemcpyHostToDevice), fn);
    if (set_regrets || set_strategy_sum) RS_HIP(hipDeviceSynchronize(), fn);
    return RS_OK;
}
// a Discounted CFR tick on the gadget rows, on the table's stream behind rs_discount_dcfr's
static int br_cfr_gadget_discount(BrRun &run, float d_pos, float d_neg, float d_sum) {
    if (run.gadget < 0) return RS_OK;
    const uint32_t cells = 2u * run.side[1 - run.gadget].n_hands;
    hipLaunchKernelGGL(k_br_gadget_discount, dim3(grid1(cells)), dim3(kBrBlock), 0, run.t->stream, run.d_g_regret, run.d_g_ssum, cells, d_pos, d_neg, d_sum);
    RS_HIP(hipGetLastError(), "rs_range_cfr_train: the gadget's tick");
    return RS_OK;
}

}  // namespace rs

struct rs_range_cfr {
    rs::BrRun *run = nullptr;
    rs_table *table = nullptr;
    int mode = 0;
};

extern "C" {

int rs_range_cfr_create(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                        size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_cfr_params *params, rs_range_cfr **out) {
    return rs_range_cfr_create_locked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, nullptr, nullptr, params, out);
}
int rs_range_cfr_create_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                                 size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_range_cfr_params *params,
                                 rs_range_cfr **out) {
    return rs_range_cfr_create_locked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, nullptr, params, out);
}
int rs_range_cfr_create_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                               size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks,
                               const rs_range_cfr_params *params, rs_range_cfr **out) {
    return rs_range_cfr_create_raked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, locks, nullptr, params, out);
}
int rs_range_cfr_create_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                              size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks,
                              const rs_rake *rake, const rs_range_cfr_params *params, rs_range_cfr **out) {
    if (!out) return fail(RS_ERR_INVALID, "rs_range_cfr_create: NULL argument");
    *out = nullptr;
    if (!t) return fail(RS_ERR_INVALID, "rs_range_cfr_create: NULL argument");
    if (int rc_ = rs::br_check_rake(rake)) return rc_;   // before the table is settled: a refused call writes nothing
    if (int rc_ = rs::br_check_weights(weights, n_hands_p0, n_hands_p1)) return rc_;
    if (int rc_ = rs::br_check_locks(locks, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1)) return rc_;
    if (int rc_ = rs::table_settle(t, false)) return rc_;   // a held pair sweep first (rs_iterate): the index kernels go to the table's stream
    const int mode = params ? params->mode : 0;
    if (mode != 0 && mode != RS_UPD_RMPLUS) return fail(RS_ERR_INVALID, "rs_range_cfr_create: params->mode is 0 or RS_UPD_RMPLUS");
    if (params && (params->sorted < RS_FORM_DEFAULT || params->sorted > RS_FORM_OFF)) return fail(RS_ERR_INVALID, "rs_range_cfr_create: params->sorted is an RS_FORM_* value");
    if (t->dtype != RS_F32)
        return fail(RS_ERR_UNSUPPORTED, "rs_range_cfr_create: RS_F32 tables only (the sums are per-deal probabilities times pots: no integer scale, and binary16 cells are out of scope)");
    rs::BrRun *run = nullptr;
    if (int rc = rs::br_prepare(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, !params || params->sorted != RS_FORM_OFF, weights,
                                &run, locks))
        return rc;
    if (int rc = rs::br_cfr_mark(run)) {
        rs::br_free(run);
        return rc;
    }
    rs::br_set_rake(run, rake);
    rs_range_cfr *s = new (std::nothrow) rs_range_cfr;
    if (!s) {
        rs::br_free(run);
        return fail(RS_ERR_OOM, "rs_range_cfr_create");
    }
    s->run = run;
    s->table = t;
    s->mode = mode;
    *out = s;
    return RS_OK;
}
void rs_range_cfr_destroy(rs_range_cfr *s) {
    if (!s) return;
    rs::br_free(s->run);
    delete s;
}
int rs_range_cfr_iterate(rs_range_cfr *s, int traverser, double *value) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_iterate: NULL argument");
    return rs::br_cfr_sweep(s->run, traverser, s->mode == RS_UPD_RMPLUS, value);
}
int rs_range_cfr_train(rs_range_cfr *s, uint64_t iterations, const rs_dcfr_params *dcfr, double *values) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_train: NULL argument");
    return rs::br_cfr_train(s->run, s->table, s->mode == RS_UPD_RMPLUS, iterations, dcfr, values);
}
int rs_range_cfr_set_gadget(rs_range_cfr *s, int resolver, const double *alt) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget: NULL argument");
    return rs::br_cfr_set_gadget(s->run, RS_GADGET_RESOLVE, resolver, alt);
}
int rs_range_cfr_set_gadget_kind(rs_range_cfr *s, int kind, int resolver, const double *alt) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_set_gadget_kind: NULL argument");
    return rs::br_cfr_set_gadget(s->run, kind, resolver, alt);
}
int rs_range_cfr_gadget_margins(const rs_range_cfr *s, double *out) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_margins: NULL argument");
    return rs::br_cfr_gadget_margins(s->run, out);
}
int rs_range_cfr_gadget_get(const rs_range_cfr *s, float *regrets, float *strategy_sum) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_get: NULL argument");
    return rs::br_cfr_gadget_rows(s->run, regrets, strategy_sum, nullptr, nullptr, "rs_range_cfr_gadget_get");
}
int rs_range_cfr_gadget_set(rs_range_cfr *s, const float *regrets, const float *strategy_sum) {
    if (!s) return fail(RS_ERR_INVALID, "rs_range_cfr_gadget_set: NULL argument");
    return rs::br_cfr_gadget_rows(s->run, nullptr, nullptr, regrets, strategy_sum, "rs_range_cfr_gadget_set");
}
size_t rs_range_cfr_bytes(const rs_range_cfr *s) { return s ? rs::br_held_bytes(s->run) : 0; }
int rs_range_cfr_launches(const rs_range_cfr *s) { return s ? rs::br_last_launches(s->run) : -1; }

}  // extern "C"

namespace rs {

// iterations of (traverser 0's sweep, traverser 1's); with Discounted CFR a tick after iteration t (counted from dcfr->t0) when t % interval == 0 and t <= cap
int br_cfr_train(BrRun *run, rs_table *t, int rmplus, uint64_t iterations, const rs_dcfr_params *dcfr, double *values) {
    if (dcfr) {
        if (dcfr->interval == 0) return fail(RS_ERR_INVALID, "rs_range_cfr_train: dcfr->interval must be > 0");
        float probe[3];
        if (int rc = rs_dcfr_factors(dcfr->alpha, dcfr->beta, dcfr->gamma, 1, probe)) return rc;
    }
    uint64_t it = dcfr ? dcfr->t0 : 0;
    for (uint64_t k = 0; k < iterations; ++k) {
        for (int p = 0; p < 2; ++p)
            if (int rc = br_cfr_sweep(run, p, rmplus, values && k + 1 == iterations ? values + p : nullptr)) return rc;
        ++it;
        if (dcfr && it <= dcfr->cap && it % dcfr->interval == 0) {
            float f[3];
            if (int rc = rs_dcfr_factors(dcfr->alpha, dcfr->beta, dcfr->gamma, it / dcfr->interval, f)) return rc;
            if (int rc = rs_discount_dcfr(t, f[0], f[1], f[2])) return rc;
            if (int rc = br_cfr_gadget_discount(*run, f[0], f[1], f[2])) return rc;
        }
    }
    return RS_OK;
}

}  // namespace rs

extern "C" {

int rs_best_response_rounds(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, int mode, double *out) {
    return rs_best_response_weighted(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, nullptr, mode, out);
}

int rs_best_response_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                              size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode, double *out) {
    return rs_best_response_locked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, nullptr, mode, out);
}

size_t rs_node_lock_size(const rs_tree *tree, int n_board0, size_t n_hands_actor, int node) { return rs::br_lock_layout(tree, n_board0, n_hands_actor, node, nullptr); }

int rs_best_response_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, int mode,
                            double *out) {
    return rs_best_response_raked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, locks, nullptr, mode, out);
}

int rs_best_response_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                           size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                           int mode, double *out) {
    if (!out) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    const bool sorted = (mode & RS_BR_SORTED) != 0;
    mode &= ~RS_BR_SORTED;
    if (int rc = rs::br_check_mode(mode & ~(RS_BR_REAL | RS_BR_CURRENT), (mode & RS_BR_REAL) != 0)) return rc;
    if (int rc = rs::br_check_rake(rake)) return rc;
    if (int rc = rs::br_check_locks(locks, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1)) return rc;   // before anything is allocated
    rs::BrRun *run = nullptr;
    if (int rc = rs::br_prepare(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, sorted, weights, &run, locks)) return rc;
    rs::br_set_rake(run, rake);
    const int rc = rs::br_execute(run, mode, out);
    rs::br_free(run);
    return rc;
}

int rs_best_response_hands(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                           size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                           int mode, int traverser, double *value, double *mass) {
    if (!value) return fail(RS_ERR_INVALID, "rs_best_response_hands: NULL argument");
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_best_response_hands: traverser is 0 or 1");
    const bool sorted = (mode & RS_BR_SORTED) != 0;
    mode &= ~RS_BR_SORTED;
    if (int rc = rs::br_check_mode(mode & ~(RS_BR_REAL | RS_BR_CURRENT), (mode & RS_BR_REAL) != 0)) return rc;
    if (int rc = rs::br_check_rake(rake)) return rc;
    if (int rc = rs::br_check_locks(locks, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1)) return rc;   // before anything is allocated
    rs::BrRun *run = nullptr;
    if (int rc = rs::br_prepare(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, sorted, weights, &run, locks)) return rc;
    rs::br_set_rake(run, rake);
    const int rc = rs::br_hands(run, mode, traverser, value, mass);
    rs::br_free(run);
    return rc;
}

size_t rs_node_report_size(const rs_tree *tree, int n_board0, size_t n_hands_traverser, const int32_t *nodes, size_t n_nodes, uint64_t *offsets) {
    return rs::br_report_layout(tree, n_board0, n_hands_traverser, nodes, n_nodes, offsets);
}

int rs_node_report(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                   size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out,
                   size_t out_doubles) {
    return rs_node_report_weighted(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, nullptr, mode, traverser, nodes, n_nodes, out,
                                   out_doubles);
}

int rs_node_report_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode, int traverser, const int32_t *nodes,
                            size_t n_nodes, double *out, size_t out_doubles) {
    return rs_node_report_locked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, nullptr, mode, traverser, nodes, n_nodes, out,
                                 out_doubles);
}

int rs_node_report_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                          size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, int mode, int traverser,
                          const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    return rs_node_report_raked(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, weights, locks, nullptr, mode, traverser, nodes, n_nodes,
                                out, out_doubles);
}

int rs_node_report_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                         size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                         int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    if (!out) return fail(RS_ERR_INVALID, "rs_node_report: NULL argument");
    const bool sorted = (mode & RS_BR_SORTED) != 0;
    mode &= ~RS_BR_SORTED;
    if (int rc = rs::br_report_check_mode(mode, traverser)) return rc;
    if (int rc = rs::br_check_rake(rake)) return rc;
    if (int rc = rs::br_check_locks(locks, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1)) return rc;   // before anything is allocated
    const size_t total = rs::br_report_layout(tree, n_board0, traverser == 0 ? n_hands_p0 : n_hands_p1, nodes, n_nodes, nullptr);   // before the game is prepared: a bad request costs nothing
    if (!total) return RS_ERR_INVALID;
    if (out_doubles < total) return fail(RS_ERR_INVALID, "rs_node_report: the output buffer is too small (rs_node_report_size doubles)");
    rs::BrRun *run = nullptr;
    if (int rc = rs::br_prepare(t, tree, board0, n_board0, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cluster, n_rounds, sorted, weights, &run, locks)) return rc;
    rs::br_set_rake(run, rake);
    const int rc = rs::br_report(run, mode, traverser, nodes, n_nodes, out, out_doubles);
    rs::br_free(run);
    return rc;
}

// the single-round game on a full board (the configuration the reference ships): NB = 1
int rs_best_response(rs_table *t, const rs_tree *tree, const uint8_t *board, const uint8_t *hands_p0, size_t n_hands_p0, const uint32_t *cluster_p0,
                     const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *cluster_p1, int mode, double *out) {
    if (!t || !tree || !board || !hands_p0 || !hands_p1 || !cluster_p0 || !cluster_p1 || !out) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    for (const rs_tree_node &n : tree->nodes)
        if (n.kind == RS_NODE_PUBLIC_CHANCE) return fail(RS_ERR_UNSUPPORTED, "rs_best_response: a single-round tree (multi-round games: rs_best_response_rounds)");
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < i; ++j)
            if (board[i] >= 52 || board[i] == board[j]) return fail(RS_ERR_INVALID, "rs_best_response: the board is five distinct cards");
    const uint32_t *cl[2] = {cluster_p0, cluster_p1};
    return rs_best_response_rounds(t, tree, board, 5, hands_p0, n_hands_p0, hands_p1, n_hands_p1, cl, 1, mode, out);
}

}  // extern "C"
