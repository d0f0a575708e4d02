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
// Three files: every kernel and what kernels take is in rs_br_dev.hpp, compiled here and launched from here alone; what needs no device (the run-outs, the raked payoffs,
// the shapes of locks and reports, every refusal of arguments as such) is in rs_br_game.cpp; this file holds the prepared game, the walks and the C entries.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <memory>
#include <vector>

#include "rs_br_dev.hpp"

#pragma clang fp contract(off)

using namespace rs;

#define RS_HIP(call, what)                                   \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return rs::hip_fail(e_, what); \
    } while (0)

namespace rs {

static unsigned grid1(uint32_t n) { return (n + kBrBlock - 1) / kBrBlock ? (n + kBrBlock - 1) / kBrBlock : 1; }

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

namespace rs {

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

// a kBrMass job: the leaf kernels of the run's showdown mode on the reach row q, as an uncontested leaf worth `value`, into the lane row v
static BrJob br_mass_job(const double *q, double *v, double value = 1.0) {
    BrJob j{};
    j.q = q;
    j.v = v;
    j.uncontested = 1;
    j.value = value;
    return j;
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

// What ONE walk is asked to do.  It lives in the call that asks (br_execute, br_hands, br_report, br_cfr_sweep) and goes down by reference: a prepared game is kept between
// calls, and nothing of a finished call -- least of all a pointer to its locals -- stays behind in it.
struct BrCall {
    int mode = RS_BR_AVERAGE;
    bool real = false;             // RS_BR_REAL: the traverser's info sets are (prefix, hand), its own nodes go to k_br_own_real_*
    bool current = false;          // RS_BR_CURRENT: get_strategy of the regrets where the walk reads a strategy
    int cfr_rmplus = 0;            // RS_UPD_RMPLUS of a full-width sweep
    const std::vector<int> *report_slot = nullptr;   // a node report (br_report): per tree node its place in the request, -1 = not asked for
    const uint64_t *report_off = nullptr;     // ... where every requested node's block starts in d_report
    double *d_report = nullptr;               // ... the call's output buffer on the device
    // rs_best_response_hands (br_hands): the root's mass row [n_pad] and the output [2][n_hands of the traverser] on the device
    double *d_hands_mass = nullptr, *d_hands_out = nullptr;
    size_t report_nodes() const { return report_slot ? size_t(std::count_if(report_slot->begin(), report_slot->end(), [](int k) { return k >= 0; })) : 0; }
};

struct BrRun {
    size_t dev_bytes = 0;                     // the ledger of its device buffers: dalloc's (the game-only half) and the walk's workspace (br_held_bytes)
    rs_table *t = nullptr;
    const rs_tree *tree = nullptr;
    bool sorted = false;           // RS_BR_SORTED: showdowns by rank order
    bool raked = false;            // rs_rake with rate > 0 and cap > 0: the tree's terminals pay by rs_rake_payoffs and their leaf jobs go to the RAKED kernels
    rs_rake rake{};                // ... the rake, as given
    bool cfr = false;              // the object is a full-width solver's (br_cfr_sweep): pi buffers in the workspace, own nodes go to k_br_cfr_own*
    double *d_pi0[2] = {nullptr, nullptr};    // ... the traverser's own reach at the root: 1.0 on every lane (the node report's as well)
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
    // node locks (rs_node_locks): per tree node its lock's rows [A][prefixes of its round][hands of the acting player] on the device (dalloc: the game-only half), nullptr =
    // not locked; empty when the game has no lock at all
    std::vector<const double *> lock_of;
    const double *lock_at(size_t id) const { return lock_of.empty() ? nullptr : lock_of[id]; }
    bool takes_pi(const BrCall &c) const { return cfr || c.report_slot; }   // the traverser's own reach goes down beside q
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
    BrKind own_kind(const BrCall &c, int r) const {
        const BrSide &me = side[p];
        if (cfr) return br_wave_per_info_set(me.n, me.n_clusters[r]) ? kBrOwnCfrWave : kBrOwnCfrThread;   // (no groups, no columns: a follow-up once a profile asks)
        if (c.real) return kBrOwnReal;   // whatever the abstraction's lists would have asked for
        if (ws_levels && c.mode == RS_BR_MAX && me.grouped[r]) return kBrOwnGrouped;
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
    int build_plan(const BrCall &c, BrPlan &pl) {
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
            if (p == gadget) {   // the resolver's sweep: the opponent enters the tree with its FOLLOW share, the rest meets the TERMINATE leaf
                BrJob jg{};
                jg.q = op.d_init_q;
                jg.q_out = d_g_qf;
                jg.v = d_g_qt;
                add(kBrGadgetReach, 0, 0, jg);
                q_in[0] = d_g_qf;
                // (max-margin has no TERMINATE leaf: the hand choice sits in the opponent's reach)
                if (gadget_kind == RS_GADGET_RESOLVE) add(kBrMass, 0, 0, br_mass_job(d_g_qt, d_g_row[p], -1.0));
            } else {             // the opponent's sweep: the root's mass row, then the gadget's own node over the root row
                // (max-margin reads M, folded once per arming: br_mm_mass)
                if (gadget_kind == RS_GADGET_RESOLVE) add(kBrMass, 0, 0, br_mass_job(op.d_init_q, d_g_row[p]));
                BrJob jo{};
                jo.v = pl.root;
                jo.sum_src[0] = d_g_row[p];
                add(kBrGadgetOwn, 0, 0, jo);
            }
        }
        if (c.d_hands_out) {   // rs_best_response_hands: the root's mass row and the fold of both root rows, behind the root's value job in either tree order
            add(kBrMass, 0, 0, br_mass_job(op.d_init_q, c.d_hands_mass));
            BrJob jf{};
            jf.v = pl.root;
            jf.sum_src[0] = c.d_hands_mass;
            jf.q_out = c.d_hands_out;
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
                if (takes_pi(c)) {
                    double *pch = ws_levels ? slot(size_t(n.n_children) * me.n_pad) : pi_level[size_t(d)];
                    add(kBrLockReach, r, id, lock_reach(lock, r, me, pi_in[id], pch, j.n_children));
                    j.q = pi_in[id];
                    for (int a = 0; a < n.n_children; ++a) pi_in[size_t(n.children[a])] = pch + size_t(a) * me.n_pad;
                }
                add(kBrLockValue, r, id, j);
                for (int a = 0; a < n.n_children; ++a) q_in[size_t(n.children[a])] = q_in[id];
            } else if (int(n.player) == p) {
                const BrKind kind = own_kind(c, r);
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
                if (takes_pi(c)) {   // its children's pi on the way down; the update (the report) reads the pi that came in
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
            if (c.report_slot && (*c.report_slot)[id] >= 0) {   // after the node's value job (kinds sort behind kBrSum within the node's step): its buffers are alive in both orders
                double *mass = ws_levels ? slot(me.n_pad) : mass_level[size_t(d)];
                add(kBrMass, r, id, br_mass_job(q_in[id], mass));
                BrJob jr{};
                jr.vch = vch;
                jr.v = v_out[id];
                jr.n_children = uint32_t(n.n_children);
                jr.q = pi_in[id];
                jr.sum_src[0] = mass;
                jr.q_out = c.d_report + c.report_off[size_t((*c.report_slot)[id])];
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
            if (e.kind == kBrGadgetReach || e.kind == kBrGadgetOwn || e.kind == kBrHands || (e.kind == kBrMass && (cfr || c.d_hands_out))) {
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
    void launch(const BrCall &c, BrKind kind, int r, const BrJob *d_jobs, uint32_t nj, const BrJob *h) {
        if (err != hipSuccess) return;
        const BrSide &me = side[p], &op = side[1 - p];
        const hipStream_t s = t->stream;
        const int mode = c.mode, cfr_rmplus = c.cfr_rmplus;
        const void *ssum = (c.current || cfr) ? t->d_regrets.get() : t->d_ssum.get();   // what the strategy readers read: the average strategy's array or the current one's
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
    void one(const BrCall &c, const BrPlan &pl, int at) { launch(c, pl.entries[size_t(at)].kind, pl.entries[size_t(at)].round, job_table + at, 1, &pl.jobs[size_t(at)]); }
    // depth first: a node's launches around its children's
    void walk(const BrCall &c, const BrPlan &pl, int id) {
        if (err != hipSuccess) return;
        const rs_tree_node &n = tree->nodes[size_t(id)];
        if (n.kind != RS_NODE_TERMINAL && n.kind != RS_NODE_ACTION) return walk(c, pl, n.children[0]);   // chance nodes pass through (cfr.rs:306-313)
        const bool own = n.kind == RS_NODE_ACTION && int(n.player) == p;
        if (!own) one(c, pl, pl.job_at[size_t(id)]);   // a leaf, or the reach of an opponent node's children
        else if (pl.own_reach_at[size_t(id)] >= 0) one(c, pl, pl.own_reach_at[size_t(id)]);   // full-width sweep, node report: the traverser's own reach of its children
        if (n.kind == RS_NODE_TERMINAL) return;
        for (int a = 0; a < n.n_children; ++a) walk(c, pl, n.children[a]);
        one(c, pl, own ? pl.job_at[size_t(id)] : pl.sum_at[size_t(id)]);
        if (pl.report_at[size_t(id)] >= 0) {   // node report: while the depth's buffers are this node's
            one(c, pl, pl.mass_at[size_t(id)]);
            one(c, pl, pl.report_at[size_t(id)]);
        }
    }

    // one traverser's pass: the plan, one upload of its jobs, the launches in the tree order the workspace was made for, the root's values back
    int run_traverser(const BrCall &c, double *root_host) {
        BrPlan pl;
        if (int rc = build_plan(c, pl)) return rc;
        n_launches = 0;
        if (job_table.bytes() < pl.jobs.size() * sizeof(BrJob)) err = job_table.alloc(pl.jobs.size());   // (no pass is in flight: each ends with a stream synchronise)
        if (err == hipSuccess) err = hipMemcpyAsync(job_table, pl.jobs.data(), pl.jobs.size() * sizeof(BrJob), hipMemcpyHostToDevice, t->stream);
        if (!ws_levels) {   // the gadget's jobs above the root (a resolver's sweeps only), the tree between them
            if (pl.gadget_reach_at >= 0) one(c, pl, pl.gadget_reach_at);
            walk(c, pl, 0);
            if (pl.gadget_mass_at >= 0) one(c, pl, pl.gadget_mass_at);
            if (pl.gadget_own_at >= 0) one(c, pl, pl.gadget_own_at);
            if (pl.hands_at >= 0) one(c, pl, pl.hands_at);
        } else {   // reach downwards by depth, the leaves in slices of 16 384, values upwards by depth: the plan's order
            for (size_t lo = 0, hi; lo < pl.jobs.size() && err == hipSuccess; lo = hi) {
                const size_t most = pl.entries[lo].kind == kBrLeaf || pl.entries[lo].kind == kBrMass ? 16384 : pl.jobs.size();
                for (hi = lo + 1; hi < pl.jobs.size() && hi - lo < most && pl.entries[hi].key == pl.entries[lo].key; ++hi) {}
                launch(c, pl.entries[lo].kind, pl.entries[lo].round, job_table + lo, uint32_t(hi - lo), &pl.jobs[lo]);
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
    int traverse(const BrCall &c, int traverser, std::vector<double> &root, double *total);
};

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

int br_prepare(rs_table *t, const BrGame &game, bool sorted, BrRun **prepared) {
    const rs_tree *const tree = game.tree;
    const uint8_t *const board0 = game.board0, *const *const hands = game.hands;
    const size_t *const n_hands = game.n_hands;
    const int n_board0 = game.n_board0, n_rounds = game.n_rounds;
    const rs_node_locks *const locks = game.locks;   // checked by the caller: br_check_locks
    if (!t || !tree || !board0 || !hands[0] || !hands[1] || !game.cluster || !prepared) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    *prepared = nullptr;
    if (int rc = br_check_weights(game)) return rc;
    if (tree->nodes.empty()) return fail(RS_ERR_INVALID, "rs_best_response: empty tree");
    if (n_board0 < 3 || n_board0 > 5) return fail(RS_ERR_INVALID, "rs_best_response: the initial board has 3, 4 or 5 cards (state.rs:59-64)");
    const int K = 5 - n_board0, D = 52 - n_board0;
    if (n_rounds < 1 || n_rounds > K + 1 || n_rounds > RS_MAX_ROUNDS) return fail(RS_ERR_INVALID, "rs_best_response: 1 .. (6 - board cards) betting rounds");
    if (n_hands[0] == 0 || n_hands[1] == 0 || n_hands[0] > 1326 || n_hands[1] > 1326) return fail(RS_ERR_INVALID, "rs_best_response: 1..1326 hands per range");
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
    run.raked = game.rake && game.rake->rate > 0.0 && game.rake->cap > 0.0;   // checked by the caller: br_check_rake
    if (run.raked) run.rake = *game.rake;
    run.NB = uint32_t(NB);
    run.n_board0 = n_board0;
    for (int r = 0; r < RS_MAX_ROUNDS; ++r) run.per_prefix[r] = uint32_t(per_prefix[r]);
    run.d_bmask = run.upload(bmask);
    uint8_t *d_boards = run.upload(cards);
    uint32_t *d_cnt0 = game.weights ? nullptr : run.upload(cnt0);   // (weighted ranges: Z0 takes its place, br_weighted_rows)
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
            const uint32_t *src = game.cluster[size_t(r) * 2 + size_t(p)];
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
    if (game.weights) {
        br_weighted_rows(run, *game.weights, mask[0], bmask, pb);
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

// the walk's workspace: allocated by the first walk and kept with the object (see br_execute)
// A node report wants more than a best response's walk left behind -- the traverser's own reach rows, a mass row per requested node (level plan) or depth -- and trades a
// workspace that lacks them for a larger one; the walks that follow run on that (they take less of it).
static int br_ensure_workspace(BrRun &run, const BrCall &call) {
    const bool pi = run.takes_pi(call);
    const size_t mass_rows = call.report_nodes();
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
int BrRun::traverse(const BrCall &c, int traverser, std::vector<double> &root, double *total) {
    if (int rc = br_ensure_workspace(*this, c)) return rc;
    last_level_plan = ws_levels;
    p = traverser;
    if (cfr) ++t->epoch;   // whatever happens below, rows may have been written
    if (int rc = run_traverser(c, root.data())) return rc;
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

// What every walk on a prepared game opens with, once the call's own arguments have passed: the object is of the kind the call is for (`cfr`: a full-width solver's), the
// table's rows are settled, the device is set, the error and the launch count of the call before are gone.  root: the root row's host copy.
static int br_open(BrRun &run, bool cfr, const char *fn, std::vector<double> &root) {
    if (run.cfr != cfr) return fail(RS_ERR_INVALID, cfr ? "rs_range_cfr: NULL argument" : std::string(fn) + ": the prepared game belongs to a full-width solver");
    if (int rc = table_settle(run.t)) return rc;
    RS_HIP(hipSetDevice(run.t->device), "hipSetDevice");
    run.err = hipSuccess;
    run.last_launches = 0;
    root.resize(run.n_pad_max);
    return RS_OK;
}
// mode (without RS_BR_SORTED) as a call of the best response proper; refuses what br_check_mode refuses
static int br_call_of_mode(int mode, BrCall &call) {
    call.real = (mode & RS_BR_REAL) != 0;
    call.current = (mode & RS_BR_CURRENT) != 0;
    call.mode = mode & ~(RS_BR_REAL | RS_BR_CURRENT);
    return br_check_mode(call.mode, call.real);
}

// the walk: both traversers against the table as it stands
int br_execute(BrRun *prepared, int mode, double *out) {
    if (!prepared || !out) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    BrCall call;
    if (int rc = br_call_of_mode(mode, call)) return rc;
    BrRun &run = *prepared;
    // The level plan wants a buffer per tree edge (full 1 176-combo ranges from a flop on the 706-node tree: 59 GB, and an allocation of that size takes seconds; 200 combos: 10 GB)
    // and buys launches, not kernel time (4 300 -> 66 per call; at full ranges both orders spend 0.24-0.27 s in their kernels): it is taken while it fits kBrLevelPlanBytes and half
    // of the free memory, else the depth-first walk runs with its two buffers per tree depth.  The workspace is allocated by the first call and KEPT with the object
    // (br_workspace_bytes / br_release_workspace: a trainer holds one object per showdown mode).
    std::vector<double> root;
    if (int rc = br_open(run, false, "rs_best_response", root)) return rc;
    for (int p = 0; p < 2; ++p)
        if (int rc = run.traverse(call, p, root, &out[p])) return rc;
    return RS_OK;
}

// One traverser's walk with the root's mass row and the fold of both root rows behind the root's value job (rs_best_response_hands): value[h] and mass[h] of the
// traverser's hands, mass may be NULL.  Everything that can refuse has refused before the first launch, and the outputs are written after the last copy has come back.
int br_hands(BrRun *prepared, int mode, int traverser, double *value, double *mass) {
    if (!prepared || !value) return fail(RS_ERR_INVALID, "rs_best_response_hands: NULL argument");
    BrCall call;
    if (int rc = br_call_of_mode(mode, call)) return rc;
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_best_response_hands: traverser is 0 or 1");
    BrRun &run = *prepared;
    std::vector<double> root;
    if (int rc = br_open(run, false, "rs_best_response_hands", root)) return rc;
    const size_t n = run.side[traverser].n_hands;
    DevBuf<double> d_mass, d_out;
    RS_HIP(d_mass.alloc(run.side[traverser].n_pad), "rs_best_response_hands: the mass row");
    RS_HIP(d_out.alloc(2 * n), "rs_best_response_hands: the output buffer");
    call.d_hands_mass = d_mass;
    call.d_hands_out = d_out;
    std::vector<double> host(2 * n);
    double total = 0.0;
    if (int rc = run.traverse(call, traverser, root, &total)) return rc;   // synchronises: nothing queued touches the two buffers after it
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
// One traverser's RS_BR_AVERAGE walk with its own reach taken down beside q, the report jobs of the requested nodes behind their value jobs; the output buffer lives on
// the device for the call and comes back in one copy.  Everything that can refuse has refused before the first launch: a refused call leaves `out` alone.
int br_report(BrRun *prepared, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    if (!prepared || !out) return fail(RS_ERR_INVALID, "rs_node_report: NULL argument");
    if (int rc = br_report_check_mode(mode, traverser)) return rc;
    BrRun &run = *prepared;
    std::vector<uint64_t> offsets(n_nodes);
    const size_t total = br_report_layout(run.tree, run.n_board0, run.side[traverser].n_hands, nodes, n_nodes, offsets.data());
    if (!total) return RS_ERR_INVALID;
    if (out_doubles < total) return fail(RS_ERR_INVALID, "rs_node_report: the output buffer is too small (rs_node_report_size doubles)");
    std::vector<int> slot_of(run.tree->nodes.size(), -1);
    for (size_t k = 0; k < n_nodes; ++k) slot_of[size_t(nodes[k])] = int(k);
    std::vector<double> root;
    if (int rc = br_open(run, false, "rs_node_report", root)) return rc;
    if (int rc = br_root_reach(run, "rs_node_report: the root reach")) return rc;
    DevBuf<double> d_out;
    RS_HIP(d_out.alloc(total), "rs_node_report: the output buffer");
    BrCall call;
    call.current = (mode & RS_BR_CURRENT) != 0;
    call.report_slot = &slot_of;
    call.report_off = offsets.data();
    call.d_report = d_out;
    double value = 0.0;
    if (int rc = run.traverse(call, traverser, root, &value)) return rc;   // synchronises: nothing queued touches d_out after it
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
    std::vector<double> root;
    if (int rc = br_open(run, true, "rs_range_cfr", root)) return rc;
    if (int rc = br_root_reach(run, "rs_range_cfr: the root reach")) return rc;
    if (run.gadget >= 0 && run.gadget_kind == RS_GADGET_MAXMARGIN && !run.g_M_ready)   // the first sweep since arming, whichever traverser's
        if (int rc = br_mm_mass(run)) return rc;
    BrCall call;
    call.cfr_rmplus = rmplus ? 1 : 0;
    double total = 0.0;
    if (int rc = run.traverse(call, traverser, root, &total)) return rc;
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
    const BrCall call;   // a leaf launch of its own, outside any walk: nothing of a call is read
    if (int rc = br_ensure_workspace(run, call)) return rc;
    const int O = 1 - run.gadget;
    run.p = O;
    const BrJob jm = br_mass_job(run.side[run.gadget].d_init_q, run.d_g_row[O]);
    if (run.job_table.bytes() < sizeof(BrJob)) run.err = run.job_table.alloc(1);
    if (run.err == hipSuccess) run.err = hipMemcpyAsync(run.job_table, &jm, sizeof(BrJob), hipMemcpyHostToDevice, run.t->stream);
    run.launch(call, kBrMass, 0, run.job_table, 1, &jm);
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

// What the one-shot entries share once their own NULL, traverser and mode checks have passed, in the order the refusals are pinned in: rake, locks, `request` (what the entry
// can refuse of its request before the game is prepared: a bad one costs nothing), br_prepare's own checks; then `walk` on the prepared game, which is freed whatever it returns.
template <typename Request, typename Walk>
static int br_one_shot(rs_table *t, const BrGame &game, int mode, Request &&request, Walk &&walk) {
    if (int rc = br_check_rake(game.rake)) return rc;
    if (int rc = br_check_locks(game)) return rc;   // before anything is allocated
    if (int rc = request()) return rc;
    BrRun *run = nullptr;
    if (int rc = br_prepare(t, game, (mode & RS_BR_SORTED) != 0, &run)) return rc;
    const int rc = walk(run, mode & ~RS_BR_SORTED);
    br_free(run);
    return rc;
}
static int br_no_request() { return RS_OK; }
static int br_check_entry_mode(int mode) { return br_check_mode(mode & ~(RS_BR_SORTED | RS_BR_REAL | RS_BR_CURRENT), (mode & RS_BR_REAL) != 0); }

// the four rs_best_response_rounds / _weighted / _locked / _raked entries
static int best_response(rs_table *t, const BrGame &game, int mode, double *out) {
    if (!out) return fail(RS_ERR_INVALID, "rs_best_response: NULL argument");
    if (int rc = br_check_entry_mode(mode)) return rc;
    return br_one_shot(t, game, mode, br_no_request, [&](BrRun *run, int m) { return br_execute(run, m, out); });
}

// the four rs_node_report* entries
static int node_report(rs_table *t, const BrGame &game, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    if (!out) return fail(RS_ERR_INVALID, "rs_node_report: NULL argument");
    if (int rc = br_report_check_mode(mode & ~RS_BR_SORTED, traverser)) return rc;
    const auto request = [&] {
        const size_t total = br_report_layout(game.tree, game.n_board0, game.n_hands[traverser], nodes, n_nodes, nullptr);
        if (!total) return int(RS_ERR_INVALID);
        return out_doubles < total ? fail(RS_ERR_INVALID, "rs_node_report: the output buffer is too small (rs_node_report_size doubles)") : int(RS_OK);
    };
    return br_one_shot(t, game, mode, request, [&](BrRun *run, int m) { return br_report(run, m, traverser, nodes, n_nodes, out, out_doubles); });
}

}  // namespace rs

struct rs_range_cfr {
    rs::BrRun *run = nullptr;
    rs_table *table = nullptr;
    int mode = 0;
};

// the four rs_range_cfr_create* entries
static int range_cfr_create(rs_table *t, const rs::BrGame &game, const rs_range_cfr_params *params, rs_range_cfr **out) {
    if (!out) return fail(RS_ERR_INVALID, "rs_range_cfr_create: NULL argument");
    *out = nullptr;
    if (!t) return fail(RS_ERR_INVALID, "rs_range_cfr_create: NULL argument");
    if (int rc_ = rs::br_check_rake(game.rake)) return rc_;   // before the table is settled: a refused call writes nothing
    if (int rc_ = rs::br_check_weights(game)) return rc_;
    if (int rc_ = rs::br_check_locks(game)) return rc_;
    if (int rc_ = rs::table_settle(t, false)) return rc_;   // a held pair sweep first (rs_iterate): the index kernels go to the table's stream
    const int mode = params ? params->mode : 0;
    if (mode != 0 && mode != RS_UPD_RMPLUS) return fail(RS_ERR_INVALID, "rs_range_cfr_create: params->mode is 0 or RS_UPD_RMPLUS");
    if (params && (params->sorted < RS_FORM_DEFAULT || params->sorted > RS_FORM_OFF)) return fail(RS_ERR_INVALID, "rs_range_cfr_create: params->sorted is an RS_FORM_* value");
    if (t->dtype != RS_F32)
        return fail(RS_ERR_UNSUPPORTED, "rs_range_cfr_create: RS_F32 tables only (the sums are per-deal probabilities times pots: no integer scale, and binary16 cells are out of scope)");
    rs::BrRun *run = nullptr;
    if (int rc = rs::br_prepare(t, game, !params || params->sorted != RS_FORM_OFF, &run)) return rc;
    if (int rc = rs::br_cfr_mark(run)) {
        rs::br_free(run);
        return rc;
    }
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

// the game of an entry's leading arguments; what the entry does not take stays NULL
#define RS_BR_GAME(...) rs::BrGame{tree, board0, n_board0, {hands_p0, hands_p1}, {n_hands_p0, n_hands_p1}, cluster, n_rounds, __VA_ARGS__}

extern "C" {

int rs_range_cfr_create(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                        size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_cfr_params *params, rs_range_cfr **out) {
    return range_cfr_create(t, RS_BR_GAME(), params, out);
}
int rs_range_cfr_create_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                                 size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_range_cfr_params *params,
                                 rs_range_cfr **out) {
    return range_cfr_create(t, RS_BR_GAME(weights), params, out);
}
int rs_range_cfr_create_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                               size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks,
                               const rs_range_cfr_params *params, rs_range_cfr **out) {
    return range_cfr_create(t, RS_BR_GAME(weights, locks), params, out);
}
int rs_range_cfr_create_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                              size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks,
                              const rs_rake *rake, const rs_range_cfr_params *params, rs_range_cfr **out) {
    return range_cfr_create(t, RS_BR_GAME(weights, locks, rake), params, out);
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

int rs_best_response_rounds(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, int mode, double *out) {
    return rs::best_response(t, RS_BR_GAME(), mode, out);
}
int rs_best_response_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                              size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode, double *out) {
    return rs::best_response(t, RS_BR_GAME(weights), mode, out);
}
int rs_best_response_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, int mode,
                            double *out) {
    return rs::best_response(t, RS_BR_GAME(weights, locks), mode, out);
}
int rs_best_response_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                           size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                           int mode, double *out) {
    return rs::best_response(t, RS_BR_GAME(weights, locks, rake), mode, out);
}

int rs_best_response_hands(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                           size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                           int mode, int traverser, double *value, double *mass) {
    if (!value) return fail(RS_ERR_INVALID, "rs_best_response_hands: NULL argument");
    if (traverser != 0 && traverser != 1) return fail(RS_ERR_INVALID, "rs_best_response_hands: traverser is 0 or 1");
    if (int rc = rs::br_check_entry_mode(mode)) return rc;
    return rs::br_one_shot(t, RS_BR_GAME(weights, locks, rake), mode, rs::br_no_request, [&](rs::BrRun *run, int m) { return rs::br_hands(run, m, traverser, value, mass); });
}

int rs_node_report(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                   size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out,
                   size_t out_doubles) {
    return rs::node_report(t, RS_BR_GAME(), mode, traverser, nodes, n_nodes, out, out_doubles);
}
int rs_node_report_weighted(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode, int traverser, const int32_t *nodes,
                            size_t n_nodes, double *out, size_t out_doubles) {
    return rs::node_report(t, RS_BR_GAME(weights), mode, traverser, nodes, n_nodes, out, out_doubles);
}
int rs_node_report_locked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                          size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, int mode, int traverser,
                          const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    return rs::node_report(t, RS_BR_GAME(weights, locks), mode, traverser, nodes, n_nodes, out, out_doubles);
}
int rs_node_report_raked(rs_table *t, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                         size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                         int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles) {
    return rs::node_report(t, RS_BR_GAME(weights, locks, rake), mode, traverser, nodes, n_nodes, out, out_doubles);
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
