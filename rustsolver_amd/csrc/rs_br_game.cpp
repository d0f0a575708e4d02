// rs_br_game.cpp -- the host-only half of the best response (rs_br.hip): the run-outs of a board, the raked payoffs, the shapes of a lock and of a node report, and every
// refusal that needs nothing but the arguments.  No device call: a change here recompiles no kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rs_internal.hpp"

namespace rs {

// run-outs of an initial board in the enumeration order of the lanes: the first new card most significant, cards ascending among those still in the deck
size_t enumerate_runouts(const uint8_t *board0, int n_board0, std::vector<uint8_t> *out) {
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

// rs_range_weights as the header states them; NULL = no weights.  Touches nothing: the weighted entry points call it before anything is allocated or written
int br_check_weights(const BrGame &game) {
    const rs_range_weights *weights = game.weights;
    const size_t n_hands[2] = {game.n_hands[0], game.n_hands[1]};
    if (!weights) return RS_OK;
    if (weights->deal != RS_DEAL_SEQUENTIAL && weights->deal != RS_DEAL_JOINT) return fail(RS_ERR_INVALID, "rs_range_weights: deal is RS_DEAL_SEQUENTIAL or RS_DEAL_JOINT");
    if (weights->reserved != 0) return fail(RS_ERR_INVALID, "rs_range_weights: reserved must be 0");
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
size_t br_lock_layout(const rs_tree *tree, int n_board0, size_t n_hands, int node, size_t *prefixes) {
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

int br_check_locks(const BrGame &game) {
    const rs_node_locks *locks = game.locks;
    if (!locks || locks->n == 0) return RS_OK;
    const rs_tree *tree = game.tree;
    const uint8_t *const board0 = game.board0, *const hands[2] = {game.hands[0], game.hands[1]};
    const size_t n_hands[2] = {game.n_hands[0], game.n_hands[1]};
    const int n_board0 = game.n_board0;
    if (!tree || !board0 || !hands[0] || !hands[1] || !locks->nodes || !locks->sigma) return fail(RS_ERR_INVALID, "rs_node_locks: NULL argument");
    if (n_board0 < 3 || n_board0 > 5) return fail(RS_ERR_INVALID, "rs_node_locks: the initial board has 3, 4 or 5 cards");
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

int br_check_mode(int mode /* without RS_BR_SORTED, RS_BR_REAL and RS_BR_CURRENT */, bool real) {
    if (mode != RS_BR_MAX && mode != RS_BR_AVERAGE)
        return fail(RS_ERR_INVALID, "rs_best_response: mode is RS_BR_MAX or RS_BR_AVERAGE (| RS_BR_SORTED, | RS_BR_CURRENT, RS_BR_MAX | RS_BR_REAL)");
    if (real && mode != RS_BR_MAX)
        return fail(RS_ERR_INVALID, "rs_best_response: RS_BR_REAL goes with RS_BR_MAX (the average strategy lives in the abstraction: RS_BR_AVERAGE | RS_BR_REAL means nothing)");
    return RS_OK;
}

// blocks of the requested nodes: offsets[k] doubles into the output, (A + 3) rows of [prefixes of the node's round][n_hands]; 0 and rs_last_error on bad arguments
size_t br_report_layout(const rs_tree *tree, int n_board0, size_t n_hands, const int32_t *nodes, size_t n_nodes, uint64_t *offsets) {
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

int br_report_check_mode(int mode /* without RS_BR_SORTED */, int traverser) {
    if (mode != RS_BR_AVERAGE && mode != (RS_BR_AVERAGE | RS_BR_CURRENT))
        return fail(RS_ERR_INVALID, "rs_node_report: the report is of the strategy profile itself: mode is RS_BR_AVERAGE (| RS_BR_CURRENT, | RS_BR_SORTED)");
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_node_report: traverser is 0 or 1");
    return RS_OK;
}

}  // namespace rs

extern "C" {

size_t rs_br_runouts(const uint8_t *board0, int n_board0, uint8_t *out_cards) {
    if (!board0 || n_board0 < 3 || n_board0 > 5) return 0;
    std::vector<uint8_t> cards;
    const size_t nb = rs::enumerate_runouts(board0, n_board0, out_cards ? &cards : nullptr);
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

size_t rs_node_lock_size(const rs_tree *tree, int n_board0, size_t n_hands_actor, int node) { return rs::br_lock_layout(tree, n_board0, n_hands_actor, node, nullptr); }

size_t rs_node_report_size(const rs_tree *tree, int n_board0, size_t n_hands_traverser, const int32_t *nodes, size_t n_nodes, uint64_t *offsets) {
    return rs::br_report_layout(tree, n_board0, n_hands_traverser, nodes, n_nodes, offsets);
}

}  // extern "C"
