/*
 * rustsolver_amd.h -- C ABI of the MI355X-native CFR regret/strategy-update engine.
 *
 * This is the drop-in boundary for RustSolver's hot path.  The reference has no FFI of its own
 * (it is a single Rust crate); every entry point below replaces a crate-internal Rust item and
 * cites it (paths relative to the reference repository root).  The Rust-side binding a
 * maintainer would add is shown in INTEGRATION.md and rust/ffi.rs (generated from this header by
 * tools/gen_rust_ffi.py).  Bench / test diagnostics (synthetic fills, HIP-event profiling, the
 * stream probe, compile-only checks of the generated kernels, table checksums) are NOT part of
 * the drop-in surface: they live in rustsolver_amd_diag.h.
 *
 * Conventions
 *   - plain C: opaque handles, pointers and sizes only; no C++/torch types;
 *   - every call returns an int status (RS_OK = 0, negative = error); rs_last_error() gives the
 *     text for the calling thread.  Where the reference panics (index out of bounds, invalid
 *     board mask, ...) this library returns an error instead;
 *   - the caller owns every host buffer; pointers named d_* are DEVICE pointers (from
 *     rs_dmalloc or the caller's own hipMalloc on the same device);
 *   - one rs_table lives on one GPU and owns one HIP stream; all calls on a table (and on
 *     solvers built on it) are enqueued on that stream in call order.  Calls that return
 *     host data synchronise the stream; the others are asynchronous;
 *   - thread-safe across different tables, not for concurrent calls on the same table;
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point fails
 *     with RS_ERR_HIP.
 *
 * Data layout in HBM: per action node two arrays  regrets[A][pitch]  and
 * strategy_sum[A][pitch]; the fast axis is the LANE  lane = board * n_clusters + cluster  of
 * that node's round, pitch = rs_table_lane_pitch() >= n_boards*n_clusters (multiple of 64).
 * Every per-lane device vector passed through this ABI (utilities, reach, strategies) uses
 * the same pitch:  float buf[pitch]  or  float buf[A][pitch].
 */
#ifndef RUSTSOLVER_AMD_H
#define RUSTSOLVER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 6   /* 2: rs_deal_batch.d_prune, rs_deal_trainer_params.prune_threshold, tiled node blocks (rs_table_tile_lanes); 3: rs_get_infosets, diagnostics split into rustsolver_amd_diag.h;
                              4: rs_kernel_forms inside rs_solver_params, rs_table_params + rs_table_create_with, rs_deal_trainer_params.prefetch, f32 deal batches;
                              5: rs_kernel_forms without `worklist` and RS_FAN_LOOP / RS_SHADOW_WIDE, with direct_rows and kept_records (same size: a zeroed struct means what it meant);
                                 rs_hand_index_verify, rs_deal_trainer_br_bytes / _br_release / _br_launches, RS_ERR_MISMATCH;
                              6: rs_deal_trainer_params.table_dtype (was `reserved`: zero = RS_I32 means what it meant), float deal tables RS_F16 and RS_UPD_RMPLUS,
                                 rs_solver_exchange_bytes (diagnostics), data-parallel sweeps keep direct rows;
                                 still 6: Discounted CFR (rs_dcfr_params, rs_dcfr_params_default, rs_dcfr_factors, rs_discount_dcfr, rs_train_dcfr, rs_solver_dcfr_fused,
                                 rs_deal_trainer_set_dcfr) -- additions only, nothing that existed changes size or meaning;
                                 still 6: RS_BR_REAL (a mode bit of rs_best_response, rs_best_response_rounds, rs_deal_trainer_best_response) -- modes without it mean what they meant;
                                 still 6: full-width CFR over hand ranges (rs_range_cfr_*, rs_deal_trainer_range_cfr) and RS_BR_CURRENT, a mode bit of the same three -- additions only;
                                 still 6: the node report (rs_node_report_size, rs_node_report, rs_deal_trainer_node_report) -- additions only;
                                 still 6: weighted hand ranges (rs_range_weights, RS_DEAL_*, rs_best_response_weighted, rs_node_report_weighted, rs_range_cfr_create_weighted) --
                                 additions only: the calls without weights take the code path they took;
                                 still 6: safe subgame re-solving: rs_tree_subtree, the re-solving gadget of a full-width solver (rs_range_cfr_set_gadget,
                                 rs_range_cfr_gadget_get, rs_range_cfr_gadget_set) -- additions only: an object without a gadget builds the plan it built and returns the bits it
                                 returned;
                                 still 6: node locks (rs_node_locks, rs_node_lock_size, rs_best_response_locked, rs_node_report_locked, rs_range_cfr_create_locked) -- additions
                                 only: a call without locks builds the plan it built and returns the bits it returned;
                                 still 6: rake (rs_rake, rs_rake_payoffs, rs_best_response_raked, rs_node_report_raked, rs_range_cfr_create_raked) -- additions only: a call
                                 without rake runs the code it ran and returns the bits it returned;
                                 still 6: weighted dealing (rs_deal_weights_*, rs_deals_sample_weighted, rs_deal_trainer_set_weights) -- additions only: rs_deals_sample and a
                                 trainer without weights launch the kernel they launched and deal the bits they dealt;
                                 still 6: the max-margin gadget and per-hand best-response values (rs_range_cfr_set_gadget_kind, rs_range_cfr_gadget_margins,
                                 rs_best_response_hands) -- additions only: rs_range_cfr_set_gadget and every walk without them launch what they launched;
                                 still 6: rake on the deal path (rs_solver_create_deals_raked, rs_deal_trainer_set_rake) -- additions only: a deal solver and a trainer without
                                 rake generate the kernel sources they generated and return the bits they returned */
#define RS_MAX_ACTIONS 8
#define RS_MAX_ROUNDS 3
#define RS_MAX_SIZES 4
#define RS_MAX_PLAYERS 2

typedef struct rs_table rs_table;
typedef struct rs_tree rs_tree;
typedef struct rs_solver rs_solver;
typedef struct rs_comm rs_comm;

/* ---- status ------------------------------------------------------------------------------ */
enum {
    RS_OK = 0,
    RS_ERR_INVALID = -1,     /* bad argument (NULL, negative size, mismatched shapes) */
    RS_ERR_OOB = -2,         /* node / board / cluster index out of bounds (Rust: index panic) */
    RS_ERR_OOM = -3,         /* host or device allocation failed */
    RS_ERR_HIP = -4,         /* HIP runtime error or no usable GPU */
    RS_ERR_UNSUPPORTED = -5, /* combination not implemented (e.g. prune on float tables) */
    RS_ERR_COMM = -6,        /* RCCL error */
    RS_ERR_MISMATCH = -7     /* a self-check found a disagreement (rs_hand_index_verify) */
};
const char *rs_last_error(void);
int rs_abi_version(void);
int rs_device_count(int *out);

/* ---- public tree: tree.rs, nodes.rs, tree_builder.rs, state.rs, options.rs ------------------
 * The tree stays on the host.  Either adopt the tree the Rust side already built
 * (rs_tree_from_nodes) or let this library rebuild it from Options (rs_tree_build reproduces
 * build_game_tree, tree_builder.rs:9-143, including the pre-order ActionNode.index numbering
 * and the valid_actions child order Check, Call, Fold, Bet.., Raise.., state.rs:125-157). */
enum { RS_NODE_PRIVATE_CHANCE = 0, RS_NODE_PUBLIC_CHANCE = 1, RS_NODE_ACTION = 2, RS_NODE_TERMINAL = 3 }; /* nodes.rs:46-52 */
enum { RS_TERM_ALLIN = 0, RS_TERM_SHOWDOWN = 1, RS_TERM_UNCONTESTED = 2 };                                /* nodes.rs:16-21 */
enum { RS_ACT_BET = 0, RS_ACT_RAISE = 1, RS_ACT_CHECK = 2, RS_ACT_CALL = 3, RS_ACT_FOLD = 4 };            /* action_abstraction.rs:4-10 */

typedef struct rs_tree_node {
    int32_t kind;                       /* RS_NODE_* */
    int32_t parent;                     /* -1 for the root (tree.rs:22) */
    int32_t n_children;
    int32_t children[RS_MAX_ACTIONS];   /* tree.rs:21, child i = action i */
    int32_t index;                      /* ActionNode.index (nodes.rs:7), -1 otherwise */
    uint8_t player;                     /* ActionNode.player (nodes.rs:8) */
    uint8_t round_idx;                  /* ActionNode.round_idx (nodes.rs:9), relative to the first street */
    int32_t action_kind[RS_MAX_ACTIONS];/* ActionNode.actions (nodes.rs:6) */
    double action_amt[RS_MAX_ACTIONS];
    uint32_t value;                     /* TerminalNode.value = pot (nodes.rs:34) */
    int32_t ttype;                      /* TerminalNode.ttype (nodes.rs:35) */
    uint8_t last_to_act;                /* TerminalNode.last_to_act (nodes.rs:36) */
    int32_t round;                      /* TerminalNode.round / PublicChanceNode.round: 0 flop, 1 turn, 2 river */
} rs_tree_node;

typedef struct rs_options {             /* options.rs:10-28, the fields build_game_tree reads */
    uint32_t stack_sizes[RS_MAX_PLAYERS];
    uint32_t starting_pot;
    int32_t n_board_cards;              /* board_mask.count_ones(): 3 / 4 / 5 (state.rs:60-65) */
    int32_t n_rounds;                   /* action_abstraction.bet_sizes.len() */
    int32_t n_bet_sizes[RS_MAX_ROUNDS];
    double bet_sizes[RS_MAX_ROUNDS][RS_MAX_SIZES];
    int32_t n_raise_sizes[RS_MAX_ROUNDS];
    double raise_sizes[RS_MAX_ROUNDS][RS_MAX_SIZES];
} rs_options;

int rs_options_default(rs_options *out);                                   /* options::default_flop(), options.rs:52-81 */
int rs_tree_build(const rs_options *options, rs_tree **out);               /* build_game_tree, tree_builder.rs:9 */
int rs_tree_from_nodes(const rs_tree_node *nodes, int n_nodes, rs_tree **out); /* adopt a Tree<GameTreeNode> (tree.rs:14-17) */
/* The subtree below an ACTION node (anything else, or an id out of range: RS_ERR_INVALID), as rs_tree_from_nodes adopts it: the nodes in the trunk's relative order with the
 * root at 0 (parent -1), ActionNode.index renumbered 0..n_act in ascending order of the trunk's index, round_idx less the root's; the absolute `round` of chance and terminal
 * nodes and a terminal's value / ttype / last_to_act are the trunk's.  node_map (may be NULL) holds rs_tree_n_nodes(tree) entries: node_map[i] = the trunk node id of the
 * subtree's node i for i < rs_tree_n_nodes(*out), -1 in the unused tail.  The action-index map follows from it with rs_tree_get_node. */
int rs_tree_subtree(const rs_tree *tree, int node, rs_tree **out, int32_t *node_map);
void rs_tree_destroy(rs_tree *tree);
int rs_tree_n_nodes(const rs_tree *tree);
int rs_tree_n_action_nodes(const rs_tree *tree);                           /* the `n_actions` of tree_builder.rs:13 */
int rs_tree_get_node(const rs_tree *tree, int node_id, rs_tree_node *out); /* Tree::get_node, tree.rs:57 */

/* ---- info-set table: infoset.rs ---------------------------------------------------------- */
enum { RS_I32 = 0,   /* reference: Box<[i32]> regrets / strategy_sum (infoset.rs:63-67) */
       RS_F32 = 1,   /* extension: f32 tables */
       RS_F16 = 2 }; /* extension: binary16 tables, f32 arithmetic */

typedef struct rs_node_desc {           /* one row of InfosetTable = Vec<Vec<Infoset>> (infoset.rs:6) */
    uint32_t n_actions;                 /* node.children.len() (infoset.rs:33) */
    uint32_t n_clusters;                /* card_abs[round_idx].get_size(player) (infoset.rs:28-32) */
    uint32_t n_boards;                  /* README.md:31-54 [board] axis; 1 = the reference as coded */
    uint8_t player;
    uint8_t round_idx;
} rs_node_desc;

/* order of `nodes` = ActionNode.index.  Zero-initialised like Infoset::init (infoset.rs:76-81). */
int rs_table_create(const rs_node_desc *nodes, int n_nodes, int dtype, int device, rs_table **out);
/* the same with an explicit block layout: lanes per tile of a tiled node block (a power of two >= 64; 0 = the default, 16 384; UINT32_MAX = never tile) and the
 * narrowest node that is tiled (0 = the default, 2^20 lanes).  rs_table_create / rs_create_infosets use the defaults. */
typedef struct rs_table_params {
    uint32_t tile_lanes;
    uint32_t tile_min_lanes;
} rs_table_params;
int rs_table_create_with(const rs_node_desc *nodes, int n_nodes, int dtype, int device, const rs_table_params *params, rs_table **out);
/* create_infosets(n_actions, tree, card_abs) (infoset.rs:8-49): sizes from the tree, the per-round
 * cluster counts n_clusters[round_idx][player] and board counts n_boards[round_idx]. */
int rs_create_infosets(const rs_tree *tree, const uint32_t n_clusters[RS_MAX_ROUNDS][RS_MAX_PLAYERS],
                       const uint32_t n_boards[RS_MAX_ROUNDS], int dtype, int device, rs_table **out);
void rs_table_destroy(rs_table *table);

int rs_table_n_nodes(const rs_table *table);
int rs_table_node_desc(const rs_table *table, int node, rs_node_desc *out);
int rs_table_dtype(const rs_table *table);
int rs_table_device(const rs_table *table);
size_t rs_table_lane_pitch(const rs_table *table, int node);  /* elements; 0 on error */
/* Layout of a node's block inside the two table arrays, for callers that address cells themselves (everything in this ABI does it for them):
 * T = rs_table_tile_lanes(node).  T == pitch: the plain block [A][pitch].  T < pitch (nodes of at least 2^20 lanes; T = 16 384): the rows are
 * interleaved tile by tile, [pitch / T][A][T], i.e. cell (action a, lane l) is element rs_table_cell_offset(node) + ((l / T) * A + a) * T + l % T --
 * a sweep streams all rows of a node together, and rows that sit next to each other move 22-35 % faster than rows tens of MB apart. */
size_t rs_table_tile_lanes(const rs_table *table, int node);
size_t rs_table_cells(const rs_table *table);                 /* sum over nodes of n_actions * pitch */
size_t rs_table_cell_offset(const rs_table *table, int node); /* element offset of a node's block (A * pitch elements) */
size_t rs_table_bytes(const rs_table *table);                 /* device bytes of both arrays */

/* Host <-> device copies.  Element type on the host: int32_t for RS_I32, float for RS_F32 and
 * RS_F16 (converted with round-to-nearest-even).  Either pointer may be NULL to skip that array.
 * Per (node, board): host layout [A][n_clusters].  Per node: host layout [A][n_boards*n_clusters]. */
int rs_table_upload(rs_table *table, int node, int board, const void *regrets, const void *strategy_sum);
int rs_table_download(rs_table *table, int node, int board, void *regrets, void *strategy_sum);
int rs_table_upload_node(rs_table *table, int node, const void *regrets, const void *strategy_sum);
int rs_table_download_node(rs_table *table, int node, void *regrets, void *strategy_sum);

/* get-infoset: `&self.infosets[an.index][cluster_idx]` (cfr.rs:375) with its two pub fields
 * (infoset.rs:65-66); out arrays of n_actions elements (host type as above). */
int rs_get_infoset(rs_table *table, int node, int board, int cluster, void *regrets, void *strategy_sum);
int rs_set_infoset(rs_table *table, int node, int board, int cluster, const void *regrets, const void *strategy_sum);
int rs_get_strategy(rs_table *table, int node, int board, int cluster, float *out);       /* Infoset::get_strategy, infoset.rs:83-102 */
int rs_get_final_strategy(rs_table *table, int node, int board, int cluster, float *out); /* Infoset::get_final_strategy, infoset.rs:104-123 */

/* get-infoset for a batch: the info sets of lanes[0..n) (lane = board * n_clusters + cluster, HOST array) of one node in one call -- what n calls of
 * rs_get_infoset would return, host layout [A][n] per array (host type as above).  Either out pointer may be NULL. */
int rs_get_infosets(rs_table *table, int node, const uint32_t *lanes, size_t n, void *regrets, void *strategy_sum);

/* ---- device memory helpers (for hosts without their own HIP binding) ------------------------ */
int rs_dmalloc(rs_table *table, size_t bytes, void **d_out);
int rs_dfree(rs_table *table, void *d_ptr);
int rs_h2d(rs_table *table, void *d_dst, const void *src, size_t bytes);
int rs_d2h(rs_table *table, void *dst, const void *d_src, size_t bytes);
int rs_dmemset(rs_table *table, void *d_dst, int byte, size_t bytes);
int rs_sync(rs_table *table);
void *rs_stream(rs_table *table);   /* the table's hipStream_t */

/* ---- bulk kernels on one action node ---------------------------------------------------------- */
enum {
    RS_UPD_CLAMP_I64 = 0,       /* mccfr traverser block, cfr.rs:413-464: i64 add, clamp to i32 (reference scale 100.0) */
    RS_UPD_WRAP_I32 = 1,        /* cfr action block, cfr.rs:612-621: saturating `as i32`, wrapping += (reference scale 10000.0) */
    RS_UPD_ARITH_MASK = 0xff,
    RS_UPD_RMPLUS = 0x100,      /* extension: regrets floored at 0 on write (regret matching+) */
    RS_UPD_PRUNE = 0x200        /* cfr.rs:352,:379-386,:419-441: skip actions with regret <= -10 000 000 */
};

/* bulk get_strategy over every lane of a node (infoset.rs:83-102): d_strategy[A][pitch] */
int rs_regret_match_node(rs_table *table, int node, float *d_strategy);
/* bulk get_final_strategy (infoset.rs:104-123): d_strategy[A][pitch] */
int rs_final_strategy_node(rs_table *table, int node, float *d_strategy);
/* every node: d_out[rs_table_cells()] with node blocks at rs_table_cell_offset(), each a plain [A][pitch] block whatever the table's own tiling
 * (calc_br's reader, cfr.rs:669-672) */
int rs_final_strategy_all(rs_table *table, float *d_out);
/* MCCFRTrainer::calc_br exactly AS CODED (cfr.rs:629-745): out[0], out[1] = the two numbers train() prints at every discount tick
 * (cfr.rs:244-246).  Its op vectors have length 1 (cfr.rs:631), so only get_final_strategy() of bucket 0 of every action node
 * enters (cfr.rs:677-679) and a terminal pays op * (+-)pot / op (cfr.rs:703-741): a placeholder, reproduced in its f32 operation
 * order.  One gather kernel over the table, a few floats back.  Synchronises the table's stream. */
int rs_calc_br(rs_table *table, const rs_tree *tree, float *out /*[2]*/);
/* What that placeholder stands in for: out[p] = expected utility per deal, in the trainer's leaf
 * utilities (cfr.rs:314-348), of player p against the opponent's AVERAGE strategy when p plays
 *   RS_BR_MAX      a best response inside the abstraction (one action per info set = cluster), or
 *   RS_BR_AVERAGE  its own average strategy (out[0] + out[1] = 0: the game is zero-sum),
 * so (out[0] + out[1]) / 2 under RS_BR_MAX is the exploitability of the average strategy profile.
 * (With rake -- rs_best_response_raked below -- the game is GENERAL-SUM: under RS_BR_AVERAGE -(out[0] + out[1]) is the expected rake per deal, and the exploitability of a
 * profile takes two calls: ((max[0] - avg[0]) + (max[1] - avg[1])) / 2, max the RS_BR_MAX result, avg the RS_BR_AVERAGE one.)  Vector form over both ranges
 * of a single-round tree on a full board (the configuration main.rs runs): deals weigh as generate_hand draws them (cfr.rs:124-137),
 * hands[n][2] hole cards, cluster[n] = get_cluster(hole cards + board, player) of every hand, board[5].  f64 on the device, every sum
 * in a fixed order.  Host pointers; synchronises the table's stream.  RS_ERR_UNSUPPORTED for trees with public chance nodes. */
enum { RS_BR_MAX = 0, RS_BR_AVERAGE = 1,
       RS_BR_SORTED = 0x100 };   /* OR into the mode: showdown and fold leaves by RANK ORDER -- the opponent's hands of a run-out sorted by score once per call, a leaf = a
                                    difference of prefix sums of the opponent's reach over that order, corrected for the hands that hold one of the traverser's cards --
                                    O(n log n) per run-out instead of the pair loop of cfr.rs:323-347 (full 1 176-combo ranges from a flop: 3.1 s -> ~0.2 s per call).  The
                                    sums run in a fixed order of their own: equal to the pair loop within f64 rounding (1e-12 relative), identical to the oracle's sorted mode */
enum { RS_BR_REAL = 0x200 };     /* OR into RS_BR_MAX (optionally with RS_BR_SORTED): the best response in the REAL game against the abstracted average strategy.  The
                                    traverser sees its own two cards: at each of its nodes of round r every (prefix of round r, hand) pair that is a deal (the hand holds none
                                    of the prefix's new cards) takes the action with the largest sum of its lanes' counterfactual values over the run-outs of that prefix, added
                                    in ascending run-out order, first maximum; lanes whose hand holds a later card of the run-out are no deals (not added, worth 0).  The opponent
                                    plays its average strategy through cluster[...] as before; the traverser's own ids are validated but not read for its decisions.  out[p] in
                                    the same per-deal units: (out[0] + out[1]) / 2 is the exploitability of the average profile in the real game -- never below the abstract
                                    number, equal to it where every (prefix, hand) pair is a cluster of its own, and the one to compare abstractions by.  RS_BR_AVERAGE | RS_BR_REAL: RS_ERR_INVALID
                                    (the average strategy lives in the abstraction) */
enum { RS_BR_CURRENT = 0x400 };  /* OR into any of the modes above: where the walk reads a strategy it reads the CURRENT one, Infoset::get_strategy of the regrets
                                    (infoset.rs:83-102), instead of get_final_strategy of the strategy sums -- the opponent always, the traverser too under RS_BR_AVERAGE.  The
                                    exploitability and the value of the last iterate: what RM+ and Discounted CFR users look at.  Every table type; RS_BR_MAX | RS_BR_REAL | RS_BR_CURRENT allowed */
int rs_best_response(rs_table *table, const rs_tree *tree, const uint8_t *board, const uint8_t *hands_p0, size_t n_hands_p0, const uint32_t *cluster_p0,
                     const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *cluster_p1, int mode, double *out /*[2]*/);
/* The same over MULTI-ROUND trees (flop or turn start).  A lane is (run-out b, hand h): generate_hand (cfr.rs:100-143) completes the board to five cards first --
 * ordered sequences without replacement, uniform -- then draws the hands; every showdown compares seven-card hands on the full board and chance nodes pass through
 * (cfr.rs:306-313).  cluster[r * 2 + p] (HOST) = dense cluster ids of player p in betting round r, [prefixes of round r][n_hands_p]: the prefix of a run-out is its
 * first r new cards, prefixes and run-outs enumerated with the first new card most significant, cards ascending among those still in the deck (rs_br_runouts writes
 * the run-outs, [NB][5], and returns NB = 1, 48 or 2 352); entries of (prefix, hand) pairs that share a card are ignored.  RS_BR_MAX: at each of p's nodes every cluster
 * takes the action with the largest SUM of its lanes' counterfactual values over all run-outs and hands -- the best response inside the abstraction when it has perfect
 * recall, otherwise the value of a valid pure strategy of the abstracted game: a lower bound on what a responder who sees its own cards takes -- RS_BR_MAX | RS_BR_REAL
 * computes that number, the best response in the real game.  f64, fixed-order sums; synchronises. */
int rs_best_response_rounds(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                            const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, int mode, double *out /*[2]*/);
size_t rs_br_runouts(const uint8_t *board0, int n_board0, uint8_t *out_cards /* [NB][5], may be NULL */);

/* ---- node report: per-hand values, reach and mass at chosen tree nodes (an extension) -----------------
 * The range and EV view of a node, and the inputs of a subgame re-solve: what RS_BR_AVERAGE's walk of rs_best_response_rounds -- same arguments, lanes (run-out b, hand h),
 * deal weights, leaves and cluster tables -- holds at the requested action nodes for ONE traverser p, both players playing the strategy the mode names: RS_BR_AVERAGE
 * (get_final_strategy of the strategy sums) or RS_BR_AVERAGE | RS_BR_CURRENT (get_strategy of the regrets), RS_BR_SORTED optional; every other mode is RS_ERR_INVALID.
 * The traverser's own reach pi (1.0 at the root, times sigma[a][cluster of the lane] at its own nodes) goes down beside the opponent's reach q.  For a node n of round r,
 * acted by either player, the rows are indexed by (prefix f of round r, hand h of p); a pair whose hand holds a card of the prefix has 0.0 in every row:
 *   cfv[a][f][h]  the sum of child a's value row over the run-outs of prefix f, ascending from 0.0, lanes that are no deal not added (RS_BR_REAL's fold).  At an
 *                 opponent's node child a's row already carries the opponent's probability of a;
 *   v[f][h]       the same fold of the node's own value row: sum_a sigma[a] * vch[a] (a ascending from 0.0) at an own node, the children summed in action order at an
 *                 opponent's;
 *   mass[f][h]    the same fold of pw[lane] * (sum of q_n[b][h_o] over the opponent hands that share no card with h or the run-out), q_n the opponent's reach at n: an
 *                 uncontested leaf of value 1.0 evaluated at the node, in the leaf order of the showdown mode.  cfv[a] / mass is the action's value in chips given that the
 *                 hand is there;
 *   own[f][h]     pi on the lowest run-out of the prefix on which (b, h) is a deal (pi is constant over them), 0.0 if there is none.
 * f64; every sum has one order, whichever tree order or kernel form ran.  `nodes` are tree node ids (rs_tree_get_node); RS_ERR_INVALID for an id that is out of range, no
 * action node or repeated, and for an out_doubles that is too small.  Node k's block starts at offsets[k] doubles and holds (A + 3) rows [prefixes of its round][n_hands of the
 * traverser]: cfv[0 .. A), v, mass, own.  rs_node_report_size returns the total number of doubles (0 with rs_last_error set on bad arguments).  Every table type; a training
 * loop's working copy is settled first; writes nothing to the table; a refused call leaves `out` alone; synchronises. */
size_t rs_node_report_size(const rs_tree *tree, int n_board0, size_t n_hands_traverser, const int32_t *nodes, size_t n_nodes, uint64_t *offsets /* [n_nodes], may be NULL */);
int rs_node_report(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1, size_t n_hands_p1,
                   const uint32_t *const *cluster, int n_rounds, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles);

/* ---- weighted hand ranges (an extension) -------------------------------------------------------------
 * rs_best_response_rounds, rs_node_report and rs_range_cfr_create take a range as a list of combos: every hand counts the same.  The forms below take per-hand weights
 * W0[h0], W1[h1] (f64, finite and > 0; a NULL row = 1.0 for every hand of that player) and one of two deal distributions.  A deal (b, h0, h1) exists when the run-out b, h0 and
 * h1 share no card, as without weights.
 *   RS_DEAL_SEQUENTIAL (0)  generate_hand (cfr.rs:100-143) with weighted draws: the run-out uniform over ordered completions, then player 0, then player 1 among what is left:
 *                           P(b, h0, h1) = P(b) * W0[h0] / Z0(b) * W1[h1] / Z1(b, h0),  Z0(b) = the sum of W0 over player 0's hands that avoid b,
 *                           Z1(b, h0) = the sum of W1 over player 1's hands that avoid b and h0.  Where Z1(b, h0) = 0 the lane weighs 0 and its share is lost, as without
 *                           weights when no hand of player 1 fits.  With every weight 1.0 this is the unweighted distribution bit for bit: the sums are exact integers
 *                           and (P(b) * W0[h0]) / (Z0(b) * Z1(b, h0)) is P(b) / (N0(b) * N1(b, h0)).
 *   RS_DEAL_JOINT (1)       P(b, h0, h1) = W0[h0] * W1[h1] / Z over all deals,  Z = the sum over the lanes (b, h0) that are no blocked lane, in ascending lane order, of
 *                           W0[h0] * Z1(b, h0): the product of two independent ranges with card removal -- what a re-solve from two reach vectors means (a node report's
 *                           `own` row times the prior of each traverser -> the weights of the subtree's game from the node's board).
 * Every sum runs over ascending hand (or lane) index from 0.0, hands that do not fit are not added: the results are a function of the inputs alone.  On the device player
 * 0's lanes carry (P(b) * W0[h0]) / (Z0(b) * Z1(b, h0)) (joint: W0[h0] / Z; 0.0 where Z1 = 0), player 1's lanes W1[h1] on every run-out where they carry 1.0 without
 * weights; no kernel of the walk changes.  The traverser's own reach pi still starts at 1.0: `own` of a node report stays a pure strategy reach and P of the full-width update
 * the sum of pi -- prior weights are chance, not strategy.  out[], *value, cfv, v and mass keep their per-deal units under the new distribution.
 * weights == NULL is the call without weights.  RS_ERR_INVALID for a weight that is NaN, infinite, zero or negative, a player's weight sum that is not finite, an unknown
 * `deal` and a non-zero `reserved`: refused before anything is allocated or written (`out` and the table are left alone).  A hand that is not in the range is left out of
 * the list, not given weight 0.  Duplicate combos stay allowed without RS_BR_SORTED (k copies of a hand = the hand with weight k) and refused with it.
 * The sampled trainer deals from the same two distributions once rs_deal_trainer_set_weights has attached weights (before its first batch): the weights are quantised to
 * integers (rs_deal_weights below), the device sampler draws exactly P with W = (double)q, and rs_deal_trainer_best_response, _node_report and _range_cfr then measure
 * that game -- the one that is dealt.  Without weights the trainer deals and measures the unweighted game, as before. */
enum { RS_DEAL_SEQUENTIAL = 0, RS_DEAL_JOINT = 1 };
typedef struct rs_range_weights {
    const double *w[2];   /* [n_hands_p], host; NULL = 1.0 for every hand of that player */
    int32_t deal;         /* RS_DEAL_* */
    int32_t reserved;     /* 0 */
} rs_range_weights;
int rs_best_response_weighted(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                              const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode,
                              double *out /*[2]*/);
int rs_node_report_weighted(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                            size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, int mode, int traverser, const int32_t *nodes,
                            size_t n_nodes, double *out, size_t out_doubles);

/* One traverser visit of every lane of `node` (cfr.rs:370-466 / :571-623):
 *   sigma = get_strategy(); util = sum_a utils[a]*sigma[a]; regrets / strategy_sum updated with
 *   (scale*reach)*(utils[a]-util) and (scale*reach)*sigma[a] in the arithmetic of `mode`.
 * d_action_utils[A][pitch], d_reach[pitch] (NULL = 1.0 for every lane), d_node_util[pitch] (NULL = discard). */
int rs_update_node(rs_table *table, int node, const float *d_action_utils, const float *d_reach, float scale, int mode,
                   float *d_node_util);
/* opponent / read-only visit: util = sum_a utils[a]*sigma[a] (cfr.rs:574,:588,:608-610), no table write */
int rs_node_util(rs_table *table, int node, const float *d_action_utils, float *d_node_util);
/* opponent reach: d_child_reach[A][pitch] = sigma[a] * d_reach (cfr.rs:585; NULL reach = 1.0) */
int rs_child_reach(rs_table *table, int node, const float *d_reach, float *d_child_reach);

/* discount sweep, cfr.rs:250-261: x = ((x as f32) * d) as i32 for every regret and strategy_sum */
int rs_discount(rs_table *table, float d);
/* cfr.rs:248-249: p = (tc / interval) as f32; d = p / (p + 1.0) */
float rs_discount_factor(uint64_t tc, uint64_t interval);

/* Discounted CFR (Brown & Sandholm, AAAI 2019; an extension, the reference knows the one factor above): a tick multiplies regrets > 0 by d_pos, all other regrets by
 * d_neg and strategy sums by d_sum.  rs_dcfr_factors, tick number p > 0, in double and each rounded once to f32:
 *   out[0] = pos = p^alpha / (p^alpha + 1),  out[1] = neg = p^beta / (p^beta + 1),  out[2] = sum = (p / (p + 1))^gamma.
 * alpha / beta = +INFINITY give exactly 1, -INFINITY exactly 0, for every p (a power that overflows double counts as +INFINITY); NaN exponents, a gamma that is not
 * finite and p = 0 are refused.  (1.5, 0, 2) is the paper's DCFR, (1, 1, 1) Linear CFR, beta = -INFINITY on RS_UPD_RMPLUS tables behaves like CFR+.
 * rs_discount_dcfr, per cell: i32 tables x = ((x as f32) * d) as i32 as rs_discount, f32 tables one multiply, binary16 tables the multiply in f32 and one rounding to
 * nearest even on the store; three equal factors ARE rs_discount(d), bit for bit.  With unequal factors a deal solver's kept shadow records (rs_kernel_forms.kept_records)
 * are not swept: the table's rows are brought up to date first (which ends a training loop's working-copy state, see rs_solver_training_loop), and the records are rebuilt
 * before the next sweep -- one transpose of the kept nodes per tick (profiles/dcfr.md). */
typedef struct rs_dcfr_params {
    double alpha, beta, gamma;   /* +-INFINITY allowed for alpha / beta */
    uint64_t interval;           /* a tick after iteration t when t % interval == 0; p = t / interval; > 0 */
    uint64_t cap;                /* no tick once t > cap */
    uint64_t t0;                 /* iterations done before this call: a run split in two equals one run */
    int32_t fused;               /* RS_FORM_*: apply a pending tick inside the next sweeps' row loads (rs_train_dcfr) */
    int32_t reserved;
} rs_dcfr_params;
int rs_dcfr_params_default(rs_dcfr_params *out);   /* 1.5, 0, 2, interval 1, cap UINT64_MAX, t0 0, fused RS_FORM_DEFAULT */
int rs_dcfr_factors(double alpha, double beta, double gamma, uint64_t p, float out[3]);   /* pos, neg, sum */
int rs_discount_dcfr(rs_table *table, float d_pos, float d_neg, float d_sum);

/* ---- full-width CFR over hand ranges (an extension) ----------------------------------------------
 * Chance-enumerated, vector-form CFR of the game rs_best_response_rounds measures -- same arguments, same lanes (run-out, hand), same deal weights, leaves and cluster
 * tables -- on that walk: the opponent plays get_strategy of its regrets, the traverser's own reach goes down beside the opponent's, and at the traverser's nodes every
 * info set c with a dealt lane takes, over its lanes in ascending order from 0.0 (f64),
 *   S[a] = sum of the children's values,  P = sum of the own reach,  U = sum_a sigma[a] * S[a],
 *   regret[a][c] = (float)(regret[a][c] + (S[a] - U))     (RS_UPD_RMPLUS: a result that is not > 0 becomes 0)
 *   strategy_sum[a][c] = (float)(strategy_sum[a][c] + P * sigma[a]),
 * sigma = get_strategy of the row before the write; info sets without a dealt lane and the opponent's rows keep their cells.  An iteration is traverser 0's sweep, then
 * traverser 1's (which sees player 0's new regrets).  Every sum has one order: the tables are a function of the inputs alone, whichever kernel form or tree order ran.
 * RS_F32 tables only (RS_ERR_UNSUPPORTED otherwise: per-deal probabilities times pots have no integer scale).  The object keeps the prepared game and, from the first
 * sweep on, the walk's workspace; the table and the tree must outlive it.  A sweep writes the table: a training loop's working copy is settled first and kept shadow
 * records are rebuilt before the next sampled sweep, as after rs_table_upload.
 * rs_range_cfr_iterate: one traverser's sweep; *value = the traverser's value per deal under the current profile; synchronises.
 * rs_range_cfr_train: `iterations` iterations; with dcfr, a tick after iteration t (counted from dcfr->t0) when t % interval == 0 and t <= cap:
 *   rs_discount_dcfr(rs_dcfr_factors(alpha, beta, gamma, t / interval)) -- bit-identical to the same sweeps and ticks issued one by one; `fused` is not read.
 * rs_range_cfr_bytes: device bytes held (the game-only half + the workspace).  rs_range_cfr_launches: kernel launches of the last sweep under the level plan, -1 after a
 * depth-first one (or before any). */
typedef struct rs_range_cfr rs_range_cfr;
typedef struct rs_range_cfr_params {
    int32_t mode;        /* 0 or RS_UPD_RMPLUS */
    int32_t sorted;      /* RS_FORM_*: rank-order showdown leaves (default on) or the pair loop */
    int32_t reserved[2];
} rs_range_cfr_params;
int rs_range_cfr_create(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                        const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds,
                        const rs_range_cfr_params *params /* NULL = defaults */, rs_range_cfr **out);
int rs_range_cfr_create_weighted(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                                 const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds,
                                 const rs_range_weights *weights /* NULL = rs_range_cfr_create */, const rs_range_cfr_params *params /* NULL = defaults */, rs_range_cfr **out);
void rs_range_cfr_destroy(rs_range_cfr *s);
int rs_range_cfr_iterate(rs_range_cfr *s, int traverser, double *value /* may be NULL */);
int rs_range_cfr_train(rs_range_cfr *s, uint64_t iterations, const rs_dcfr_params *dcfr /* NULL = no ticks */, double *values /* [2], last iteration's, may be NULL */);
/* ---- the re-solving gadget (Burch, Johanson, Bowling 2014: CFR-D) on a full-width solver: safe subgame re-solving ----
 * The object's game is a subgame cut out of a trunk (rs_tree_subtree, its board the node's board).  P = resolver, O = 1 - P, n = O's hand count.  Above the tree's root O decides
 * PER HAND (not per cluster: the alternative value is a per-hand number) between action 0 TERMINATE, which pays hand h alt[h] -- the value the hand had in the trunk, in chips
 * per unit of the resolver's reach mass (a node report's value / mass) -- and action 1 FOLLOW, which enters the tree.  The gadget holds f32 rows regret[2][n] and ssum[2][n]
 * in the OBJECT (the table, its descriptors and rs_create_infosets do not change), zero after set_gadget.  sigma = get_strategy of a hand's row (infoset.rs:83-102), as f64.
 *   O's sweep: the walk leaves the root's value row vF[b][h]; m[b][h] = the uncontested leaf of value 1.0 on P's initial reach (the node report's mass row at the root);
 *     vT[lane] = alt[h] * m[lane].  For every hand h with a dealt lane, over its dealt lanes (run-outs b whose cards h avoids) in ascending run-out order from 0.0:
 *       S[0] = sum vT   S[1] = sum vF   Pi = the count of dealt lanes (O's own reach is 1.0 there)
 *       U = sigma[0] * S[0] + sigma[1] * S[1]                             (a ascending from 0.0)
 *       regret[a][h] = (float)(regret[a][h] + (S[a] - U))                  (RS_UPD_RMPLUS: a result that is not > 0 becomes 0)
 *       ssum[a][h]   = (float)(ssum[a][h] + Pi * sigma[a])
 *       v[lane] = sigma[0] * vT[lane] + sigma[1] * vF[lane]                (a ascending from 0.0; 0.0 where the lane is no deal)
 *     *value = the sum of v as root rows are summed.  Hands without a dealt lane keep their cells.
 *   P's sweep: O's reach at the tree's root is init_q[lane] * sigma[1][h]; the walk and the table updates are otherwise unchanged.  *value = the root row's sum plus the sum,
 *     taken the same way, of the TERMINATE leaf's row: the uncontested leaf of value -1.0 on the reach (init_q[lane] * sigma[0][h]) * alt[h].  The gadget rows are not written.
 *   rs_range_cfr_train's Discounted CFR ticks multiply the gadget rows with the same three factors, one f32 multiply per cell.
 * rs_range_cfr_set_gadget: alt is a HOST array of n doubles; resolver not 0 / 1 or a NaN / infinite alt: RS_ERR_INVALID, nothing written.  Calling it again re-arms with the new alt
 *   (and resolver) and zeroes the rows.  rs_range_cfr_gadget_get / _set copy the rows out / in ([2][n] floats each,
 *   either may be NULL); RS_ERR_INVALID before set_gadget.  Both tree orders run the gadget through the same kernels and give the same bits. */
int rs_range_cfr_set_gadget(rs_range_cfr *s, int resolver, const double *alt /* [n_hands of player 1 - resolver], HOST */);
int rs_range_cfr_gadget_get(const rs_range_cfr *s, float *regrets /* [2][n] */, float *strategy_sum /* [2][n] */);
int rs_range_cfr_gadget_set(rs_range_cfr *s, const float *regrets, const float *strategy_sum);
/* ---- the max-margin gadget (Moravcik, Schmid, Ha, Hladik, Gaukrodger, AAAI 2016) on a full-width solver ----
 * A second gadget kind: O picks the HAND on which the resolver improved least, the resolver maximises that minimum margin.  rs_range_cfr_set_gadget_kind with
 * RS_GADGET_RESOLVE is rs_range_cfr_set_gadget in every respect; an unknown kind is RS_ERR_INVALID; the checks, the refusals (locks, rake: RS_ERR_UNSUPPORTED), the zeroing
 * of the rows and re-arming are rs_range_cfr_set_gadget's.  The rows stay regret[2][n], ssum[2][n] and _gadget_get / _set keep their layout: under RS_GADGET_MAXMARGIN row 0
 * is the hand-choice row, row 1 is never read and never written by a sweep (Discounted CFR ticks multiply both rows as before).
 *   m = the root's mass row on O's side, dealt(b, h) the deal test.  M[h] = the sum of m[b][h] over dealt lanes, b ascending from 0.0: a function of the prepared game alone,
 *     computed once per arming (in front of the first sweep, whichever traverser's) and kept on the device: no sweep launches the mass row again.  live[h] = h has a dealt lane and M[h] > 0; L = the number of live hands.
 *   rho, from row 0 as it stands, in f64 (regret matching over hands; not infoset.rs:83-102's f32 sum: n reaches 1 176):
 *     pos[h] = live[h] && regret[h] > 0 ? (double)regret[h] : 0.0;  norm = the sum of pos over h ascending from 0.0;
 *     rho[h] = pos[h] / norm if norm > 0, otherwise 1.0 / L for live hands and 0.0 for dead ones (L = 0: every rho is 0).
 *   O's sweep: the walk is unchanged (O's own reach 1.0 at the root, the table updates as always, the root row vF left as the walk wrote it).  Per live hand:
 *       F[h] = the sum of vF[b][h] over dealt lanes, ascending      u[h] = F[h] / M[h] - alt[h]
 *       U = the sum of rho[h] * u[h] over live h ascending from 0.0
 *       regret[h] = (float)((double)regret[h] + (u[h] - U))          (RS_UPD_RMPLUS: a result that is not > 0 becomes 0)
 *       ssum[h]   = (float)((double)ssum[h] + rho[h])
 *       margin[h] = alt[h] - F[h] / M[h]                              (f64, kept on the device)
 *     Dead hands keep their cells and have margin NaN.  *value = U.
 *   P's sweep: O enters the tree with q[lane] = init_q[lane] * (rho[h] / M[h]) -- one division, then one multiply; dead hands 0.0.  The walk and the table updates are
 *     otherwise unchanged, the gadget rows are not written.  *value = the root row's sum plus the sum of rho[h] * alt[h] over live h ascending from 0.0: the rho-weighted
 *     margin under the current profile.
 *   A deliberate simplification: O's in-tree regrets see values without the 1 / M[h] factor and O's in-tree strategy sums do not carry rho.  Both are a positive constant per
 *     hand, which regret matching ignores where an info set is one hand; O's subgame strategy is not what gets grafted.
 *   The sums over hands are the ascending sequential f64 sums, bit for bit, in both tree orders.
 * rs_range_cfr_gadget_margins: the margin row of the last O sweep ([n] doubles); RS_ERR_INVALID without a max-margin gadget or before O's first sweep since arming. */
enum { RS_GADGET_RESOLVE = 0, RS_GADGET_MAXMARGIN = 1 };
int rs_range_cfr_set_gadget_kind(rs_range_cfr *s, int kind, int resolver, const double *alt /* [n_hands of player 1 - resolver], HOST */);
int rs_range_cfr_gadget_margins(const rs_range_cfr *s, double *out /* [n] */);
size_t rs_range_cfr_bytes(const rs_range_cfr *s);
int rs_range_cfr_launches(const rs_range_cfr *s);

/* ---- node locks: a player's per-hand strategy fixed at chosen action nodes (an extension) ---------------
 * "At this node this player plays THIS", per hand; everything around it is solved, measured and inspected as before.  A lock of action node n (round r, A actions, acted
 * by player P) is a HOST array sigma[(a * n_prefix + f) * n_hands + h], a < A, f over the prefixes of round r in the node report's order (rs_br_runouts: the first r new
 * cards of a run-out, the first most significant), h over P's hands: the granularity of the re-solving gadget and the layout of a node report's rows, so that a lock
 * can be built from a report.  In every walk -- rs_best_response_locked, rs_node_report_locked, the sweeps of an object of rs_range_cfr_create_locked -- whichever player
 * traverses and whatever the mode, with lane = b * n_hands + h and f = b / (run-outs under a prefix of round r):
 *   P is the opponent:   child a's reach is q[lane] * sigma[a][f][h], one f64 multiply; the node's value is the sum of its children's values in action order, as without
 *                        a lock.
 *   P is the traverser:  v[lane] = sum_a sigma[a][f][h] * vch[a][lane], f64, a ascending from 0.0; 0.0 on a lane that is no deal (the hand holds a card of the run-out),
 *                        as every own node writes.  Under RS_BR_MAX (with or without RS_BR_REAL) nothing is maximised there: the result is the best response of
 *                        everything that is not locked.  A full-width sweep reads and writes neither the regret row nor the strategy-sum row of the node; the children's
 *                        own reach is pi[lane] * sigma[a][f][h].  A node report at a locked node reports cfv, mass and own as usual and v by the lock.
 * RS_BR_CURRENT / RS_BR_AVERAGE choose the table array for the nodes that are NOT locked only.  Discounted CFR ticks (rs_discount_dcfr, rs_range_cfr_train) still multiply
 * the whole table, a locked node's rows included: harmless, nothing reads them.  The rows are used as given, nothing is renormalised.  WHOLE nodes only: locking some hands
 * of a node and leaving the others free is out of scope (the free hands' info sets would need their lanes' sums without the locked lanes).
 * Checked before anything is allocated or the table is settled -- a refused call returns RS_ERR_INVALID and leaves outputs and table alone: a node id that is out of range
 * or no action node; an id given twice; a NULL row; an entry that is not finite or is < 0; |sum_a sigma[a][f][h] - 1| > 1e-9 (a ascending from 0.0) for a (prefix, hand)
 * pair that shares no card.  Pairs that do share a card are not sum-checked, and their entries are never used for a deal.
 * locks == NULL or n == 0 is the _weighted call in every respect: the same bits, the same launches, the same rs_range_cfr_bytes.  The rows are copied to the device
 * when the game is prepared (counted in rs_range_cfr_bytes) and need not outlive the call.  rs_range_cfr_set_gadget on an object created with locks returns
 * RS_ERR_UNSUPPORTED: a gadget and locks on one object are out of scope.  The rs_deal_trainer_* forms and the sampled trainer stay unlocked.
 * rs_node_lock_size: the doubles of node's lock, A * n_prefix * n_hands_actor; 0 with rs_last_error set on bad arguments; host only. */
typedef struct rs_node_locks {
    uint32_t n;                   /* locked action nodes; 0 = none */
    const int32_t *nodes;         /* [n] tree node ids (rs_tree_get_node), distinct action nodes */
    const double *const *sigma;   /* [n] HOST arrays, rs_node_lock_size doubles each */
} rs_node_locks;
size_t rs_node_lock_size(const rs_tree *tree, int n_board0, size_t n_hands_actor, int node);
int rs_best_response_locked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                            const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights,
                            const rs_node_locks *locks, int mode, double *out /*[2]*/);
int rs_node_report_locked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                          size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, int mode,
                          int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles);
int rs_range_cfr_create_locked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                               const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights,
                               const rs_node_locks *locks, const rs_range_cfr_params *params /* NULL = defaults */, rs_range_cfr **out);

/* ---- rake: raked pots in best response, node report and full-width CFR (an extension) -------------------
 * A percentage of the pot with a cap, taken from the winner at the tree's TERMINAL nodes.  For a terminal n: pot = (double)(float)n.value, the number every leaf pays,
 * and r = min(cap, rate * pot), one f64 multiply; cap = +inf means uncapped.  What traverser p is paid:
 *   RS_TERM_UNCONTESTED   p is the folder (p == last_to_act): -pot;   p is the other player: pot - r
 *   RS_TERM_SHOWDOWN, RS_TERM_ALLIN   win: vw = pot - r;   lose: vl = -pot;   tie: vt = -0.5 * r
 * A leaf row stays v[b, hp] = pw[lane] * sum over the deals (b, hp, ho), ascending ho, of q[b, ho] * u, u one of the three numbers; by rank order (RS_BR_SORTED) win and
 * lose are the sums they were, tie = (((LE - L) - (E0 - L0)) - (E1 - L1)) + q[the opponent's hand of the traverser's own two cards, if it holds it] (LE, L: the prefix sums
 * up to the traverser's score inclusive / exclusive, E_t, L_t the same among the holders of its card t) and acc = ((vw * win) + (vt * tie)) + (vl * lose) -- the level
 * plan and the depth-first walk give the same bits.  Only tree terminals are raked: the mass rows of a node report (an uncontested leaf of value 1.0) are not.
 * UNITS: a leaf pays +-pot, the WHOLE number in n.value, not the opponent's half of it.  Where both players have put in equal amounts n.value is one player's stake and
 * the chips on the table are 2 * n.value, so a room's "5 % of the pot, capped at C" is rate = 0.10, cap = 2 C here.  The library converts nothing.
 * The game becomes GENERAL-SUM: under RS_BR_AVERAGE -(out[0] + out[1]) is the expected rake per deal; the exploitability of a profile is
 * ((max[0] - avg[0]) + (max[1] - avg[1])) / 2 -- two calls.  RS_BR_REAL, RS_BR_CURRENT, weights and locks compose unchanged: a traverser's walk reads its own payoffs only.
 * Checked before anything is allocated or the table is settled -- RS_ERR_INVALID, outputs and table left alone: rate not finite, < 0 or > 1; cap NaN or < 0; a non-zero
 * reserved.  rake == NULL, rate == 0 and cap == 0 are the _locked call in every respect: the same bits, the same launches, the same rs_range_cfr_bytes.
 * rs_range_cfr_set_gadget on an object created with rake returns RS_ERR_UNSUPPORTED (the TERMINATE branch pays the resolver minus the opponent's alternative: a zero-sum
 * construction).  The sampled trainer takes the same rake through rs_solver_create_deals_raked / rs_deal_trainer_set_rake (below); the lane solvers (rs_solver_create),
 * rs_deal_trainer_calc_br and the single-round rs_best_response stay unraked.
 * rs_rake_payoffs: host only; out = {win, tie, lose} of `player` at terminal `node` -- an uncontested terminal fills all three with the player's one payoff; rake == NULL
 * gives {pot, 0, -pot} (uncontested: +-pot); a node that is no terminal, a bad player or a bad rake: RS_ERR_INVALID, out untouched. */
typedef struct rs_rake { double rate; double cap; int32_t reserved[2]; } rs_rake;
int rs_rake_payoffs(const rs_tree *tree, int node, const rs_rake *rake, int player, double out[3] /* win, tie, lose */);
int rs_best_response_raked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                           const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights,
                           const rs_node_locks *locks, const rs_rake *rake, int mode, double *out /*[2]*/);
int rs_node_report_raked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                         size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks, const rs_rake *rake,
                         int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles);
int rs_range_cfr_create_raked(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0,
                              const uint8_t *hands_p1, size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights,
                              const rs_node_locks *locks, const rs_rake *rake, const rs_range_cfr_params *params /* NULL = defaults */, rs_range_cfr **out);

/* ---- per-hand root values of the best-response walk (an extension) ----
 * rs_best_response_raked's arguments (weights, locks and rake may each be NULL), ONE traverser, every mode rs_best_response_raked accepts -- RS_BR_MAX, RS_BR_AVERAGE,
 * | RS_BR_SORTED, | RS_BR_REAL, | RS_BR_CURRENT -- with the same refusals (RS_BR_AVERAGE | RS_BR_REAL: RS_ERR_INVALID).  For hand h of the traverser, over the run-outs b
 * ascending from 0.0, a lane that is no deal not added:
 *   value[h] = the sum of the root's value row v[b][h]
 *   mass[h]  = the same fold of the root's mass row: the uncontested leaf of value 1.0 on the opponent's initial reach (the node report's mass at node 0).
 * A hand without a dealt lane gets 0.0 in both.  value[h] / mass[h] under RS_BR_MAX is the hand's counterfactual best-response value per unit of the opponent's mass: the
 * alternative value of a re-solve (rs_range_cfr_set_gadget's alt) and, measured in a re-solved subgame, the check of its margins; the sum of value is
 * rs_best_response_raked's out[traverser].  All arithmetic is f64 and every sum has one order: the level plan and the depth-first walk give the same bits.  The call
 * settles a training loop's working copy, writes nothing to the table, synchronises, and leaves value and mass alone when it refuses.  mass may be NULL. */
int rs_best_response_hands(rs_table *table, const rs_tree *tree, const uint8_t *board0, int n_board0, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                           size_t n_hands_p1, const uint32_t *const *cluster, int n_rounds, const rs_range_weights *weights, const rs_node_locks *locks,
                           const rs_rake *rake, int mode, int traverser, double *value /* [n_hands of traverser] */, double *mass /* [n_hands], may be NULL */);

/* ---- iterate: MCCFRTrainer (cfr.rs) ------------------------------------------------------------
 * Lane model: lane (board b, cluster c) is one scalar cfr() traversal (cfr.rs:481-627)
 * in which get_cluster() (cfr.rs:564-568) returns c for either player and evaluate() is replaced by
 * the leaf inputs below.  The host walks the public tree once to build a launch plan (per tree
 * depth: opponent-reach kernels top-down, node-util / update kernels bottom-up) and replays it. */
enum { RS_LEAF_UNCONTESTED = 0, /* +-pot from TerminalNode.last_to_act (cfr.rs:316-322); no buffer */
       RS_LEAF_SIGN = 1,        /* d_buf[pitch] = sign(score[0]-score[1]) of evaluate() (cfr.rs:323-347): value = +-pot / 0 */
       RS_LEAF_UTIL = 2 };      /* d_buf[pitch] = utility from the traverser's point of view, used verbatim */
enum { RS_OPP_FULL = 0,         /* cfr(): every opponent action is recursed, reach * sigma[i], util = sum (cfr.rs:576-589) */
       RS_OPP_SAMPLE = 1 };     /* mccfr(): ONE opponent action sampled from sigma with rand's WeightedIndex (cfr.rs:467-476);
                                   the random bits are a counter hash of (sweep seed, ActionNode.index, lane), the sweep seed
                                   advances by one on every rs_iterate call (sample_seed, call index) */
enum { RS_CHANCE_PASS = 0,      /* mccfr: PublicChance goes to child 0 (cfr.rs:306-309); needs equal board counts */
       RS_CHANCE_ENUM = 1 };    /* cfr: reach *= 1/len, util = sum over the len = n_boards[r+1]/n_boards[r] deals (cfr.rs:502-522) */

typedef struct rs_leaf_desc {
    int32_t kind;
    const float *d_buf;
} rs_leaf_desc;

/* Kernel-form choices a caller may legitimately make.  EVERY field: 0 = the engine's own choice (what a zeroed struct gets), so a caller that never looks at
 * this struct loses nothing.  Results are bit-identical whatever is chosen here (the GPU tests run the forms against each other and against the oracle); only
 * time and workspace change.  The remaining A/B switches of the kernel generator are test-only and come from the environment, read in one place
 * (csrc/rs_knobs.cpp). */
enum { RS_FORM_DEFAULT = 0, RS_FORM_ON = 1, RS_FORM_OFF = 2 };
enum { RS_FAN_DEFAULT = 0,   /* = RS_FAN_EXPAND */
       RS_FAN_NONE = 1,      /* lane sweeps, subtree directly below an ENUM chance node (cfr.rs:502-522): separate expand / reduce launches */
       RS_FAN_EXPAND = 2 };  /* the subtree's kernel scales the chance node's own reach row by 1/len itself: no expand launch, no per-deal reach rows */
enum { RS_SHADOW_DEFAULT = 0,   /* = RS_SHADOW_RULE */
       RS_SHADOW_RULE = 1,      /* deal sweeps: a node keeps an AoS shadow only while the batch is likely to read it (n_deals * 8 >= its cells * round subtrees) */
       RS_SHADOW_ALL = 2 };     /* a shadow for every node */
typedef struct rs_kernel_forms {
    int32_t lane_fan;           /* RS_FAN_* */
    int32_t deals_per_thread;   /* deal sweeps: 1, 2 or 4 deals per thread of the generated kernels */
    int32_t kept_records;       /* RS_FORM_*: the nodes of the rounds that `direct_rows` covers KEEP their shadow records between sweeps (wide records, one set for both
                                   traversers): the pass that adds the delta rows into the table adds them to the records too, rs_discount sweeps them as well, any other
                                   write to the table has them rebuilt before the next sweep; inside rs_train / rs_deal_trainer_train they are the working copy and the table's
                                   rows of those nodes are written back when the loop returns.  The walks then read staged rows instead of gathering a table that is too large
                                   to transpose per sweep (solve_three_street, 64 K deals against 2 GB: 1.60 -> 1.23 ms per batch, 1.28 -> 0.81 without discount ticks).
                                   Costs the records' memory (1.3x the nodes' table rows) -- and, for a host that drives rs_iterate and rs_discount ITSELF, a discount
                                   sweep over table and records both (1.6 -> 1.9 ms per batch while a tick comes every 1.5 batches, 1.3 -> 0.95 after the discount
                                   phase): such a loop should call rs_train / rs_deal_trainer_train for its batches, or switch this off for short runs.  Default: on.  (ABI 4 had `worklist` in this slot.) */
    int32_t shadow;             /* RS_SHADOW_* */
    int32_t deal_order;         /* RS_FORM_*: sampled deal sweeps walk the batch in the order of the traverser's last-round cluster id, and the last round's subtrees
                                   sum their deltas along the runs of equal cluster (DPP segmented scan) instead of LDS tiles or delta rows (default: on for multi-round
                                   trees beyond 24 K deals per batch, profiles/r04_deals.md) */
    int32_t delta_rows;         /* RS_FORM_*: i32 deal sweeps keep no delta tiles and issue no atomics inside the walk: a visit stores its deltas at the deal's LIST POSITION
                                   ([2A][batch pitch] i32 rows per traverser node, coalesced), and one streaming pass per sweep sums every row by cluster (LDS histogram of
                                   one row at a time) into the delta tables.  Applies to the round subtrees whose traverser nodes have at most 16 384 clusters */
    int32_t direct_rows;        /* RS_FORM_*: round subtrees whose traverser nodes have MORE than 16 384 clusters (lossless abstractions: 180 234 on the river) store delta rows too, and
                                   one pass per round adds them straight into the TABLE once the round's walks are done (atomic adds at the key row's clusters) -- no delta-table
                                   entries, no share of the apply pass for those nodes.  Default: on; data-parallel deal batches exchange the delta TABLES between sweep and apply
                                   and must switch it off (rs_solver_attach_comm refuses a solver that has it on; rs_deal_trainer does so for world > 1) */
    int32_t pair_sweeps;        /* RS_FORM_*: lane solvers whose traverser plans are one chance-free subtree kernel each (fused river trees, PASS chance, one rank) walk BOTH
                                   traversers per lane in one launch, every node's regrets carried in registers from the first walk to the second: 612 instead of 776 bytes per
                                   lane and iteration on the 14-node river tree.  rs_iterate(.., 0, ..) then holds its sweep until rs_iterate(.., 1, ..) (see there).  Default: on.
                                   (ABI 6 had `reserved` in this slot: a zeroed struct means what it meant.) */
} rs_kernel_forms;

typedef struct rs_solver_params {
    float scale;            /* 100.0 (cfr.rs:424) or 10000.0 (cfr.rs:617) */
    int32_t mode;           /* RS_UPD_* */
    int32_t chance_mode;    /* RS_CHANCE_* */
    int32_t use_graph;      /* 1: replay each traverser's plan as one hipGraph launch */
    int32_t fuse_subtrees;  /* 1: every chance-free subtree is walked by ONE tree-specialised straight-line kernel per
                               traverser, generated from the tree and compiled at create time with hipRTC: utilities and
                               reaches stay in registers, only table rows and leaf rows touch HBM.  0: level-by-level node
                               kernels.  Results are bit-identical either way. */
    int32_t opp_mode;       /* RS_OPP_* */
    uint64_t sample_seed;   /* RS_OPP_SAMPLE: base seed of the sweep-seed sequence */
    /* Multi-GPU sharding of a multi-round RS_CHANCE_ENUM sweep (BASELINE configs[3]); shard_world <= 1 = off.
     * The boards of round `shard_round` (and of every later round) are split contiguously over the ranks, sizes differing
     * by at most one; earlier rounds are REPLICATED.  This table holds only the rank's boards:
     * n_boards[shard_round] = hi - lo with lo = rank*base + min(rank, rem), base = shard_global_boards / shard_world.
     * At every chance node entering shard_round the ranks exchange the utility rows of their boards (one all-gather),
     * after which each rank sums all deals in the reference order and applies IDENTICAL updates to the replicated
     * rounds: results equal the single-GPU sweep bit for bit, for any rank count. */
    int32_t shard_world;
    int32_t shard_rank;
    int32_t shard_round;
    uint32_t shard_global_boards;   /* boards of shard_round over all ranks */
    /* Data-parallel deal batches (rs_solver_create_deals on a REPLICATED table, one rank per GPU): the global index of this rank's
     * first deal inside the union batch.  Only the opponent-sampling hash sees it, so that a deal draws the same bits whichever
     * rank owns it.  With a communicator attached rs_iterate sweeps, all-reduces the i32 deltas (ncclInt32 sum) and applies the
     * union: N ranks x n deals equal ONE GPU with N*n deals per batch, bit for bit. */
    uint32_t deal_offset;
    rs_kernel_forms forms;  /* zeroed = the engine's choices */
} rs_solver_params;

/* leaves_p0 / leaves_p1: one entry per TREE node id (only terminals are read) for traverser 0 / 1;
 * pass the same array twice unless RS_LEAF_UTIL buffers differ per traverser. */
int rs_solver_create(rs_table *table, const rs_tree *tree, const rs_leaf_desc *leaves_p0, const rs_leaf_desc *leaves_p1,
                     const rs_solver_params *params, rs_solver **out);   /* MCCFRTrainer::init, cfr.rs:159-184 */
/* Deal batches: lanes are DEALS.  Every deal carries, per (round_idx, player), the dense cluster id that
 * ICardAbstraction::get_cluster() returned for it (card_abstraction.rs:204-209, :245-251, :287-293; cfr.rs:361-365) and
 * the table keeps the reference's own shape  infosets[an.index][cluster_idx]  (n_boards = 1; cluster counts may differ
 * per player and round).  Several deals of a batch may address the same info set, which the reference lets race
 * (cfr.rs:414); here the sweep is BATCH-SYNCHRONOUS and deterministic: every deal reads the table as it was when the
 * sweep started, its update becomes the i32 delta (new - old) against the value it read, deltas are accumulated with
 * atomic adds (wrapping, order-independent) and applied when the sweep ends.  RS_CHANCE_PASS (one run-out per deal,
 * cfr.rs:306-313).  Float tables (RS_F32, RS_F16: extensions, fuse_subtrees = 1, no RS_UPD_PRUNE, any number of clusters per round; under a communicator the ranks exchange per-deal delta items and sum them in global deal
 * order inside rs_iterate, rs_iterate_phase refuses them): a visit's deltas
 * (scale*reach)*(u - util) and (scale*reach)*sigma are f32, every cell's deltas are added IN DEAL ORDER from 0.0 and then to
 * the cell -- one rounding to the table's type per cell and sweep, and with RS_UPD_RMPLUS the traverser's regrets that do
 * not end the sweep above 0 end it at 0.  Leaf buffers and d_root_util hold one float per deal, pitch = round_up(n_deals, 64);
 * cluster-id vectors have the same pitch (padding ignored). */
typedef struct rs_deal_batch {
    uint32_t n_deals;
    const uint32_t *d_cluster[RS_MAX_ROUNDS][RS_MAX_PLAYERS];   /* device; [round_idx][player] */
    const uint8_t *d_prune;   /* RS_UPD_PRUNE only: device [pitch] bytes, 1 = this deal is traversed with prune = true.  In train() pruning is a
                                 property of the DEAL (cfr.rs:213-221: t > PRUNE_THRESHOLD && q > 0.05); NULL = every deal */
} rs_deal_batch;
int rs_solver_create_deals(rs_table *table, const rs_tree *tree, const rs_deal_batch *deals, const rs_leaf_desc *leaves_p0,
                           const rs_leaf_desc *leaves_p1, const rs_solver_params *params, rs_solver **out);
/* The same with raked pots (rs_rake above): an RS_LEAF_SIGN leaf pays the traverser (float)(pot - r) where it wins, (float)(-0.5 r) on a tie and (float)(-pot) where it
 * loses, an uncontested terminal (float)(-pot) to the folder and (float)(pot - r) to the other player -- rs_rake_payoffs' numbers, each rounded to f32 once.  RS_LEAF_UTIL
 * buffers are used verbatim.  Three wave-uniform constants per showdown terminal and two selects in the generated round subtrees; i32, f32 and binary16 tables, every
 * rs_kernel_forms choice.  rake == NULL, rate == 0 and cap == 0 are rs_solver_create_deals in every respect: the same sources, the same bits, the same
 * rs_solver_n_launches.  Checked before anything is allocated or compiled: RS_ERR_INVALID for a rake rs_best_response_raked refuses; RS_ERR_UNSUPPORTED with
 * fuse_subtrees = 0 (the level-by-level node kernels take no rake), without hipRTC, and for a tree whose first node below the root is no action node.
 * rs_solver_attach_comm on a raked solver returns RS_ERR_UNSUPPORTED: nothing in the sweep depends on the rank, but no multi-process test holds the combination. */
int rs_solver_create_deals_raked(rs_table *table, const rs_tree *tree, const rs_deal_batch *deals, const rs_leaf_desc *leaves_p0,
                                 const rs_leaf_desc *leaves_p1, const rs_solver_params *params, const rs_rake *rake, rs_solver **out);
void rs_solver_destroy(rs_solver *solver);
/* one traverser sweep over every lane: `self.cfr(0, player, hand, 1f32, ..)` (cfr.rs:217) for all lanes.
 * d_root_util[pitch of the root round] (NULL = discard) receives the value returned at node 0.
 * Paired solvers (rs_solver_forms bit 2, rs_kernel_forms.pair_sweeps): rs_iterate(s, 0, u0) HOLDS the sweep and only records it, u0 included; the next
 * rs_iterate(s, 1, u1) runs both sweeps as one launch and writes u0 and u1.  Any other entry point that takes the solver, its table or a trainer over it (rs_sync and
 * rs_stream included, and every solver's rs_iterate on the same table) first issues a held sweep on its own, so results are those of two separate sweeps whatever
 * comes in between.  u0 must stay valid until then.  A host that launches work of its own on a stream pointer it cached earlier must call rs_sync or rs_stream first. */
int rs_iterate(rs_solver *solver, int traverser, float *d_root_util);
/* MCCFRTrainer::train (cfr.rs:188-265), deterministic: per iteration both traversers sweep, t += 1, then
 * the discount check `t > threshold` (d = p/(p+1), p = t/interval) until t > discount_cap. */
int rs_train(rs_solver *solver, uint64_t iterations, uint64_t discount_interval, uint64_t discount_cap);
/* Discounted CFR over full sweeps.  Per iteration both traversers sweep, t += 1 (starting from params->t0), and if t <= cap and t % interval == 0 a tick with
 * rs_dcfr_factors(alpha, beta, gamma, t / interval).
 * FUSED form: the tick is not swept but left pending, and the next iteration's sweeps apply it to the rows they load anyway -- traverser 0's sweep discounts player 0's
 * regrets (by sign) and strategy sums before it updates and stores them and player 1's regrets for regret matching only; traverser 1's sweep discounts player 1's rows and
 * reads player 0's as just written.  No pass over the table of its own: on the 14-node river tree 776 bytes per lane and iteration instead of 776 + 608 (or, paired,
 * 612 + 608).  Bit-identical to "rs_discount_dcfr after iteration t, then both sweeps of iteration t + 1"; a tick still pending when the call returns -- the one after the
 * last iteration included -- is swept before it does.  Who fuses: lane solvers with fuse_subtrees = 1 on one rank whose traverser plans are one chance-free subtree kernel
 * each (what makes a solver pairable), with RS_OPP_FULL and without RS_UPD_PRUNE -- only then does every sweep load every row the tick must reach.  Sampled opponents and
 * pruning leave nodes unvisited, ENUM chance nodes and the level plan spread a sweep over several kernels, deal batches share cells between lanes: all of those take
 * rs_discount_dcfr between the iterations, as does params->fused = RS_FORM_OFF.  The discounted kernels are generated and compiled on the first fused call (cached like the
 * others); a paired solver issues its two unpaired launches while the fused loop runs (there is no discounted pair kernel) and pairs again afterwards.
 * rs_solver_dcfr_fused: 1 if the last rs_train_dcfr on the solver applied its ticks inside the sweeps, 0 if it swept them. */
int rs_train_dcfr(rs_solver *solver, uint64_t iterations, const rs_dcfr_params *params);
int rs_solver_dcfr_fused(const rs_solver *solver);
/* For a host that writes MCCFRTrainer::train's loop itself (rs_iterate / rs_iterate_phase per batch, rs_discount at its ticks): on = 1 in front of the loop, on = 0 behind
 * it.  In between the solver's kept shadow records (rs_kernel_forms.kept_records) are the working copy, as they are inside rs_train and rs_deal_trainer_train: the table's rows
 * of those nodes are neither added to nor discounted until on = 0 writes them back.  Any call that reads or writes table contents in between (download, upload, strategy
 * query, best response, checkpoint, fill) writes them back itself first and ends the working-copy state -- correct, but the rest of the loop then updates table and records
 * both; a second solver sweeping the same table in between is not covered.  A solver without kept records: both calls do nothing. */
int rs_solver_training_loop(rs_solver *solver, int on);
/* Deal-batch solvers: rs_iterate_phase(.., 0) = the sweep (deltas accumulated, table untouched), (.., 1) = table += delta, delta = 0;
 * between the two the ranks' delta tables are summed (rs_comm_allreduce_deltas; tests emulate ranks and add them on the host).
 * Sharded sweeps: rs_iterate = phase 0 (everything inside the sharded rounds) + exchange + phase 1 (the replicated rounds).
 * With a communicator attached the exchange is one in-place ncclAllGather over xGMI; without one the host runs the phases
 * itself and moves the ranks' slots (tests emulate several ranks on one GPU this way). */
int rs_solver_attach_comm(rs_solver *solver, rs_comm *comm);
int rs_iterate_phase(rs_solver *solver, int traverser, int phase, float *d_root_util /* phase 1 only, may be NULL */);
/* the exchange buffer of a traverser: [shard_world][bytes_per_rank]; rank r's slot is the r-th */
int rs_solver_exchange_info(rs_solver *solver, int traverser, void **d_buf, size_t *bytes_per_rank);
int rs_comm_allgather(rs_comm *comm, rs_table *table, void *d_buf, size_t bytes_per_rank);
int rs_comm_allreduce_deltas(rs_comm *comm, rs_table *table);   /* in-place ncclInt32 sum of the table's two delta arrays */
/* the delta tables of a deal-batch table: two DEVICE i32 arrays of rs_table_cells() elements laid out like the table itself */
int rs_table_deltas(rs_table *table, int32_t **d_dregrets, int32_t **d_dstrategy_sum);
/* device memory a solver holds beside the table, EVERYTHING it allocated: the utility / reach arena; for deal sweeps the AoS shadow of the table, the packed (or ordered)
   per-deal records, the live-deal lists with their reach / position rows and counters, the work lists; the job descriptors of every launch; the exchange buffer of a
   sharded sweep.  (The table's own delta arrays of a deal solver belong to the table: rs_table_deltas.) */
size_t rs_solver_workspace_bytes(const rs_solver *solver);
int rs_jit_available(void);   /* 1 if libhiprtc.so can be loaded (needed for fuse_subtrees) */
int rs_solver_n_launches(const rs_solver *solver, int traverser);
/* which kernel forms the solver chose (rs_kernel_forms): bit 0 = deal sweeps walk the batch in last-round-cluster order (deal_order), bit 1 = some round subtree
   stores delta rows (delta_rows), bit 2 = both traversers' lane sweeps run as one pair launch (pair_sweeps; rs_solver_n_launches then counts them under traverser 0),
   bit 3 = that pair kernel is the split form (two threads of a workgroup share a lane's subtree, cut below its root); negative = bad solver */
int rs_solver_forms(const rs_solver *solver);

/* ---- card-abstraction plumbing in front of get-infoset (host only; card_abstraction.rs) -----------------------------
 * These entry points take canonical hand indices as INPUT (e.g. from the Rust side's own hand_indexer_s); the index itself is
 * computed by rs_hand_indexer / rs_card_abs further down. */
typedef struct rs_dense_map rs_dense_map;
/* bucket files: flat little-endian u32 per canonical hand index (gen_abstraction/main.rs:372-380 writes,
 * card_abstraction.rs:227-229 / :269-271 read).  *out is malloc'ed: release it with rs_free_u32. */
int rs_cluster_file_read(const char *path, uint32_t **out, size_t *n_out);
int rs_cluster_file_write(const char *path, const uint32_t *clusters, size_t n);   /* fails if the file exists (create_new) */
void rs_free_u32(uint32_t *p);
/* index_to_cluster (card_abstraction.rs:20-29); cluster_arr = NULL is the ISOMORPHIC abstraction (bucket = index) */
int rs_index_to_cluster(const uint32_t *cluster_arr, size_t arr_len, const uint64_t *indices, size_t n, uint64_t *out);
/* dense ids 0..size: generate_maps (card_abstraction.rs:75-184) in first-appearance order of `buckets` (the reference's
 * channel-arrival order is nondeterministic) */
int rs_dense_map_create(const uint64_t *buckets, size_t n, rs_dense_map **out);
void rs_dense_map_destroy(rs_dense_map *map);
size_t rs_dense_map_size(const rs_dense_map *map);                                  /* get_size, card_abstraction.rs:211-213 */
int rs_dense_map_lookup(const rs_dense_map *map, const uint64_t *buckets, size_t n, uint32_t *dense_out); /* get_cluster's map step */
int rs_dense_map_keys(const rs_dense_map *map, uint64_t *keys_out);                 /* dense id -> bucket, size() entries */

/* ---- canonical hand index: rust_poker::hand_indexer_s (Cargo.toml:18, crate not vendored) -------------------------------------
 * The suit-isomorphic index of K. Waugh, "A Fast and Optimal Hand Isomorphism Algorithm" (AAAI 2013 workshop), which the crate
 * wraps.  card = 4*rank + suit, rank 0..12 = 2..A.  A hand is its rounds' cards in order (hole cards first); cards inside a round
 * may come in any order.  The partition into classes is pinned by the reference's own numbers (1 286 792 flop hands, out.txt:1;
 * 12 888 turn clusters, card_abstraction.rs:315); the ORDER of indices follows the published algorithm and is not pinned by any
 * reference fixture. */
typedef struct rs_hand_indexer rs_hand_indexer;
/* hand_indexer_s::init(rounds, cards_per_round) (card_abstraction.rs:88-90, gen_abstraction/ehs.rs:30-33) */
int rs_hand_indexer_create(int rounds, const uint8_t *cards_per_round, rs_hand_indexer **out);
void rs_hand_indexer_destroy(rs_hand_indexer *indexer);
uint64_t rs_hand_indexer_size(const rs_hand_indexer *indexer, int round);      /* .size(round) (gen_abstraction/main.rs:91,359) */
int rs_hand_indexer_rounds(const rs_hand_indexer *indexer);
int rs_hand_indexer_n_cards(const rs_hand_indexer *indexer, int round);        /* cards of rounds 0..round */
/* .get_index(cards) for n hands (card_abstraction.rs:205); cards[n][n_cards(round)]; `round` = rounds-1 is what get_index returns */
int rs_hand_index(const rs_hand_indexer *indexer, int round, const uint8_t *cards, size_t n, uint64_t *out);
/* The index-ORDER self-check (card_abstraction.rs:204-209 get_cluster -> hand_indexer.get_index; :227-229 bucket files indexed by it): expect[i] = what the
 * caller's own indexer (rust_poker's hand_indexer_s::get_index) returned for cards[i].  RS_OK when every hand agrees; RS_ERR_MISMATCH at the first that does not
 * (*first_bad = its position, n when all agree; *got_at_first_bad = this library's index for it; either may be NULL).  Run it on ~1 000 random hands per round before
 * loading bucket files written by the reference's gen_abstraction (rust/verify_index.rs). */
int rs_hand_index_verify(const rs_hand_indexer *indexer, int round, const uint8_t *cards, size_t n, const uint64_t *expect, size_t *first_bad,
                         uint64_t *got_at_first_bad);
/* .get_hand(round, index, cards) (gen_abstraction/main.rs:117,195): one representative hand per index; cards_out[n][n_cards(round)] */
int rs_hand_unindex(const rs_hand_indexer *indexer, int round, const uint64_t *indices, size_t n, uint8_t *cards_out);
/* get_index on the GPU: d_cards[n_cards(round)][pitch] (u8, row i = card i, pitch = round_up(n, 64)), d_out[n]; asynchronous */
int rs_hand_index_device(rs_table *table, rs_hand_indexer *indexer, int round, const uint8_t *d_cards, uint32_t n, uint64_t *d_out);

/* ---- one round's card abstraction: ISOMORPHIC / EMD / OCHS (card_abstraction.rs:31-298) ----------------------------------------
 * ::init = generate_maps (card_abstraction.rs:75-184): every hand of every range x every way to complete the board to the round is
 * indexed with hand_indexer_s::init(2, [2, 3 + betting_round]), mapped through the bucket file if there is one (index_to_cluster,
 * :20-29) and given the next dense id on first sight.  hands_p*: (u8,u8) combos = HandRange.hands after remove_invalid_combos
 * (cfr.rs:161-163).  cluster_arr = NULL: ISOMORPHIC (bucket = index); otherwise the round_{r}_emd.dat / _ochs.dat contents
 * (rs_cluster_file_read), copied.  Dense ids follow first appearance in the reference's loop order (its own order is a race). */
typedef struct rs_card_abs rs_card_abs;
int rs_card_abs_create(int betting_round /* 0 flop, 1 turn, 2 river */, const uint8_t *hands_p0, size_t n_hands_p0, const uint8_t *hands_p1,
                       size_t n_hands_p1, uint64_t initial_board_mask, const uint32_t *cluster_arr, size_t arr_len, rs_card_abs **out);
void rs_card_abs_destroy(rs_card_abs *abs);
int rs_card_abs_round(const rs_card_abs *abs);
size_t rs_card_abs_size(const rs_card_abs *abs, int player);                     /* get_size (card_abstraction.rs:211-213) */
uint64_t rs_card_abs_index_size(const rs_card_abs *abs);                         /* hand_indexer.size(1): length a bucket file must have */
int rs_card_abs_keys(const rs_card_abs *abs, int player, uint64_t *keys_out);    /* dense id -> bucket, size(player) entries */
/* get_cluster(&cards, player) (card_abstraction.rs:204-209, :245-251, :287-293) for n hands on the host;
 * cards[n][5 + betting_round] = the player's hole cards, then the board (cfr.rs:357-365) */
int rs_card_abs_get_cluster(const rs_card_abs *abs, const uint8_t *cards, size_t n, int player, uint32_t *out);
/* get_cluster for every deal of a batch on the GPU.  d_cards[9][pitch] u8 as for rs_showdown_sign: rows 0-4 the board, 5-6 player 0's
 * hole cards, 7-8 player 1's.  d_cluster_p0 / d_cluster_p1 [pitch] receive the dense ids (either may be NULL): ready to be an
 * rs_deal_batch.d_cluster[round_idx][player].  Asynchronous on the table's stream.  A deal whose bucket has no dense id (Rust:
 * unwrap on None) gets id 0 and raises an error word that rs_card_abs_status reports. */
int rs_card_abs_clusters_device(rs_card_abs *abs, rs_table *table, const uint8_t *d_cards, uint32_t n_deals, uint32_t *d_cluster_p0,
                                uint32_t *d_cluster_p1);
int rs_card_abs_status(rs_card_abs *abs, rs_table *table);   /* synchronises; RS_ERR_OOB if a deal since the last call had no cluster */

/* ---- generate_hand for a batch of deals (cfr.rs:100-143) ---------------------------------------------------------------------------
 * Board cards missing from board_mask are drawn uniformly without replacement by rejection (cfr.rs:115-122), then one combo per range
 * by rejection against everything dealt (cfr.rs:126-137); Uniform::from(0..52) and slice::choose are rand 0.7's widening-multiply
 * samplers.  The random bits are a counter hash of (seed, first_deal + i) -- the reference's SmallRng is seeded from thread_rng and is
 * not reproducible.  d_hands_p*: DEVICE arrays of (u8,u8) combos.  d_cards[9][pitch] as above.  d_err (device u32, may be NULL): bit 2 is
 * raised when a deal found no valid combo within 4096 draws (the reference would loop forever). */
int rs_deals_sample(rs_table *table, uint64_t seed, uint64_t first_deal, uint64_t board_mask, const uint8_t *d_hands_p0,
                    uint32_t n_hands_p0, const uint8_t *d_hands_p1, uint32_t n_hands_p1, uint32_t n_deals, uint8_t *d_cards, uint32_t *d_err);

/* ---- weighted dealing (an extension): rs_deals_sample with per-hand weights ---------------------------------------------------------
 * The probabilities are ratios of integers, so a deal is a pure function of (seed, deal number, inputs).  rs_deal_weights holds, per player, the quanta q[i] and their
 * inclusive prefix sums cum[i], on the host and (with a table) on the table's device.  table == NULL gives a host-only object: rs_deal_weights_quanta works, the
 * sampler refuses it.  A NULL row = 1.0 for every hand.  With m the largest weight of a row, q[i] = (uint64_t)floor(w[i] / m * 4294967296.0 + 0.5) in IEEE f64, in
 * that operation order: unit weights give 2^32 each, scaling a row by a power of two changes no bit, Q = sum q < 2^43.  RS_ERR_INVALID, before anything is allocated,
 * for a weight that is NaN, infinite, zero or negative, a quantum that comes out 0 (the hand weighs less than 2^-33 of the largest: drop it from the range), n_p == 0
 * or n_p > 1326, and an unknown `deal` (RS_DEAL_SEQUENTIAL or RS_DEAL_JOINT, above).
 * A draw from a row: u uniform in [0, Q) by rand 0.7's widening multiply on a 64-bit word of the deal's counter hash (len = Q, zone = (Q << clz(Q)) - 1; a rejected
 * word consumes its counter), the hand is the first index i with u < cum[i].  Counters k = 0, 1, ... of the deal:
 *   RS_DEAL_SEQUENTIAL  the board is completed as rs_deals_sample does (same counters).  Then player 0, then player 1: up to RS_DEAL_WEIGHTED_TRIES words are spent on
 *                       draws from the player's row -- a zone-rejected word counts as one of them, a hand that shares a card with anything dealt is rejected.  If none
 *                       gives a hand the player is dealt exactly: Z = the sum of q over the hands that fit (Z == 0: the deal gives up), u' uniform in [0, Z) by the
 *                       same widening multiply on the following words, the hand is the first fitting index whose running sum of fitting quanta exceeds u'.  Both
 *                       branches draw from the same conditional law: P(b, h0, h1) = P(b) q0[h0] / Z0(b) * q1[h1] / Z1(b, h0) exactly, and a deal that exists is
 *                       always dealt, however peaked the range.
 *   RS_DEAL_JOINT       an attempt = the board completion, one draw for player 0 from its full row, one for player 1 from its full row (zone-rejected words are
 *                       redrawn).  If either hand shares a card with the board or the hands share a card the WHOLE attempt is discarded and the next begins with
 *                       fresh board cards on the next counters (redrawing the hands alone would not be the joint law).  Accepted deals have P = q0[h0] q1[h1] / Z
 *                       over all deals; an attempt is accepted with probability Z / (Q0 Q1) (sum over run-outs of P(b) times the fitting mass), and there is no
 *                       exact fallback: very peaked ranges that block each other run into the cap below.
 * Both: at most 4096 words per deal (counter 4096 stays the prune draw); giving up raises bit 2 of the error word and writes the lowest nine free cards, as
 * rs_deals_sample.  dw == NULL is rs_deals_sample, bit for bit; RS_ERR_INVALID for a dw without device rows, made for another device, or whose row lengths differ from
 * n_hands_p0 / n_hands_p1.  The object must outlive every launch that reads it (rs_sync the table before destroying it). */
#define RS_DEAL_WEIGHTED_TRIES 32
typedef struct rs_deal_weights rs_deal_weights;
int rs_deal_weights_create(rs_table *table /* may be NULL: host only */, const double *w0, size_t n0, const double *w1, size_t n1, int deal, rs_deal_weights **out);
void rs_deal_weights_destroy(rs_deal_weights *dw);
int rs_deal_weights_quanta(const rs_deal_weights *dw, int player, uint64_t *q /*[n_p]*/);
int rs_deals_sample_weighted(rs_table *table, uint64_t seed, uint64_t first_deal, uint64_t board_mask, const uint8_t *d_hands_p0, uint32_t n_hands_p0,
                             const uint8_t *d_hands_p1, uint32_t n_hands_p1, const rs_deal_weights *dw, uint32_t n_deals, uint8_t *d_cards, uint32_t *d_err);

/* train()'s per-deal prune decision (cfr.rs:213-221): d_flags[pitch] u8, 1 where deal number first_deal + i exceeds prune_threshold
 * (PRUNE_THRESHOLD = 10 000 000, cfr.rs:190) AND its `q: f32 = rng.gen()` -- counter 4096 of the deal's hash, after everything
 * generate_hand can draw -- is > 0.05.  Ready to be an rs_deal_batch.d_prune.  Asynchronous on the table's stream. */
int rs_deals_prune_flags(rs_table *table, uint64_t seed, uint64_t first_deal, uint64_t prune_threshold, uint32_t n_deals, uint8_t *d_flags);

/* ---- MCCFRTrainer on the GPU: init + train over sampled deals (cfr.rs:159-297) -----------------------------------------------------
 * Per batch, all on the table's stream: rs_deals_sample -> rs_card_abs_clusters_device for every round -> rs_showdown_sign -> one
 * sampled-opponent sweep per traverser (rs_solver_create_deals).  One deal = one reference iteration (cfr.rs:209-226). */
typedef struct rs_deal_trainer rs_deal_trainer;
typedef struct rs_deal_trainer_params {
    uint64_t board_mask;           /* Options.board_mask (options.rs:17): 3, 4 or 5 cards */
    uint32_t deals_per_batch;
    uint64_t seed;
    uint64_t discount_interval;    /* cfr.rs:190 DISCOUNT_INTERVAL (0 = never discount) */
    uint64_t discount_cap;         /* cfr.rs:240: no discount once t exceeds it */
    rs_solver_params solver;       /* scale 100, RS_UPD_CLAMP_I64, RS_OPP_SAMPLE = the reference's mccfr(); chance_mode is forced to PASS,
                                      deal_offset is set from rank */
    uint32_t world, rank;          /* data-parallel training on replicated tables: this rank deals numbers (b*world + rank)*n .. + n of
                                      global batch b; 0 / 0 or 1 / 0 = single GPU.  t advances by world * deals_per_batch per batch */
    uint64_t prune_threshold;      /* cfr.rs:190 PRUNE_THRESHOLD (10 000 000): deals numbered beyond it are traversed with prune = true when their
                                      q > 0.05 (cfr.rs:213-221, rs_deals_prune_flags); UINT64_MAX = never.  With a finite threshold the solver runs
                                      in RS_UPD_PRUNE mode with per-deal flags that stay zero (= unpruned, bit for bit) before it */
    int32_t prefetch;              /* RS_FORM_*: deal the next batch on a second stream while the current one is swept (default: on from 65 536 deals per batch for multi-round games, beyond 262 144 for one-round games) */
    int32_t table_dtype;           /* element type of the table the trainer creates: RS_I32 (0: the reference's), or -- extensions -- RS_F32 / RS_F16: float deal sweeps
                                      (rs_solver_create_deals: f32 per-deal deltas summed in deal order, one rounding per cell and sweep, any number of clusters per
                                      round, world >= 1: bit-equal to one GPU with the union batch); these need prune_threshold = UINT64_MAX.  (The field was `reserved`, zero, until ABI 5) */
} rs_deal_trainer_params;
/* MCCFRTrainer::init (cfr.rs:159-184): card_abs[round_idx] for the tree's rounds (borrowed: keep them alive), ranges as above;
 * creates the zero-filled table from the abstractions' sizes (create_infosets, cfr.rs:176) on `device`. */
int rs_deal_trainer_create(const rs_tree *tree, rs_card_abs *const *card_abs, int n_rounds, const uint8_t *hands_p0, size_t n_hands_p0,
                           const uint8_t *hands_p1, size_t n_hands_p1, const rs_deal_trainer_params *params, int device,
                           rs_deal_trainer **out);
void rs_deal_trainer_destroy(rs_deal_trainer *trainer);
rs_table *rs_deal_trainer_table(rs_deal_trainer *trainer);      /* trainer.infosets; owned by the trainer */
rs_solver *rs_deal_trainer_solver(rs_deal_trainer *trainer);
int rs_deal_trainer_train(rs_deal_trainer *trainer, uint64_t n_batches);   /* train(): deals_per_batch iterations per batch */
/* world > 1: the communicator whose all-reduce makes every rank apply the deltas of the union batch (rs_comm_create on this
 * trainer's table) */
int rs_deal_trainer_attach_comm(rs_deal_trainer *trainer, rs_comm *comm);
/* the bookkeeping that ends a batch (t += world * deals_per_batch, discount check of cfr.rs:240-262); rs_deal_trainer_train calls it,
 * callers that drive rs_deal_trainer_deal + rs_iterate_phase themselves call it once per batch */
int rs_deal_trainer_finish_batch(rs_deal_trainer *trainer);
int rs_deal_trainer_deal(rs_deal_trainer *trainer);             /* only the dealing half of a batch (cards, cluster ids, signs) */
/* synchronises; error if a deal could not be sampled / addressed since the last call.  A trainer that deals ahead (prefetch) has dealt the batch AFTER the last one it trained
 * as well -- it waits in the staging buffers for the next call -- so the report covers that batch too. */
int rs_deal_trainer_status(rs_deal_trainer *trainer);
uint64_t rs_deal_trainer_iterations(const rs_deal_trainer *trainer);   /* t of cfr.rs:200 */
/* calc_br at the discount ticks (cfr.rs:244-246 runs it before the sweep and prints the two numbers): enable != 0 makes every tick
 * call rs_calc_br first; rs_deal_trainer_last_br returns the latest pair and the iteration count it was taken at (RS_ERR_INVALID
 * before the first tick).  rs_deal_trainer_calc_br / _best_response run the two readers on the trainer's own tree, ranges and
 * abstraction at any time (best response: single-round trainers on a full board). */
int rs_deal_trainer_set_tick_br(rs_deal_trainer *trainer, int enable);
/* Discounted CFR at the trainer's ticks: WHEN a tick comes stays the reference's rule (t > threshold, discount_interval, discount_cap: cfr.rs:240-262); the sweep then
 * takes rs_dcfr_factors(alpha, beta, gamma, t / discount_interval) through rs_discount_dcfr instead of the one factor of cfr.rs:248-249 (only the exponents of `params`
 * are read).  i32, f32 and binary16 tables, with or without a communicator: the factors depend on t alone, every rank computes the same.  NULL: back to cfr.rs:248-261. */
int rs_deal_trainer_set_dcfr(rs_deal_trainer *trainer, const rs_dcfr_params *params);
/* Weighted hand ranges on the dealing stream (rs_range_weights and rs_deals_sample_weighted above).  Only before the first batch is dealt: RS_ERR_INVALID once a batch
 * has been dealt or staged.  NULL: unweighted.  Every batch is then dealt by the weighted sampler, on whichever stream deals; deal numbers do not change, so ranks that
 * set the same weights deal the union batch of one GPU.  rs_deal_trainer_best_response, _node_report and _range_cfr prepare their game with weights (double)q and the
 * same `deal`; the prepared games kept from earlier calls are dropped here. */
int rs_deal_trainer_set_weights(rs_deal_trainer *trainer, const rs_range_weights *weights);
/* Raked pots in the trainer's sweeps (rs_solver_create_deals_raked).  Only before the first batch is dealt: RS_ERR_INVALID once a batch has been dealt or staged, and for a
 * rake rs_best_response_raked refuses.  NULL (or rate == 0, cap == 0): unraked.  The trainer's solver is built again with the rake -- rs_deal_trainer_solver returns another
 * object afterwards; a refused call leaves the trainer as it was (RS_ERR_UNSUPPORTED: a solver with fuse_subtrees = 0, or a trainer with a communicator;
 * rs_deal_trainer_attach_comm on a raked trainer returns the same).  rs_deal_trainer_best_response, _node_report and _range_cfr prepare their game with the same rake, so the
 * trainer measures the general-sum game it trains; the prepared games kept from earlier calls are dropped here.  Weights and rake compose, in either order.
 * rs_deal_trainer_calc_br and the calc_br at the ticks stay unraked. */
int rs_deal_trainer_set_rake(rs_deal_trainer *trainer, const rs_rake *rake);
int rs_deal_trainer_last_br(const rs_deal_trainer *trainer, float *out /*[2]*/, uint64_t *iterations);
int rs_deal_trainer_calc_br(rs_deal_trainer *trainer, float *out /*[2]*/);
int rs_deal_trainer_best_response(rs_deal_trainer *trainer, int mode, double *out /*[2]*/);
/* rs_range_cfr_train on the trainer's own tree, ranges, board and cached cluster tables (the game rs_deal_trainer_best_response measures; RS_F32 trainers).  The prepared
 * game and its workspace stay with the trainer (counted by rs_deal_trainer_br_bytes, given back by rs_deal_trainer_br_release).  Does not advance
 * rs_deal_trainer_iterations. */
int rs_deal_trainer_range_cfr(rs_deal_trainer *trainer, uint64_t iterations, const rs_range_cfr_params *params /* NULL = defaults */,
                              const rs_dcfr_params *dcfr /* NULL = no ticks */, double *values /* [2], may be NULL */);
/* The best-response objects a trainer keeps between calls (one per showdown mode: the game-only index, and the walk's workspace -- a buffer per tree edge while that stays
 * below 16 GB, two per tree depth otherwise): the device bytes they hold, a call that gives the workspaces back (the next best response allocates them again), and the kernel
 * launches the last call made (-1: the depth-first walk ran, one or two launches per tree node). */
/* rs_node_report on the trainer's own tree, ranges, board and cached cluster tables.  The prepared game and the workspace are the objects rs_deal_trainer_best_response
 * keeps for the showdown mode (counted by rs_deal_trainer_br_bytes, given back by rs_deal_trainer_br_release); a workspace that lacks the report's rows grows. */
int rs_deal_trainer_node_report(rs_deal_trainer *trainer, int mode, int traverser, const int32_t *nodes, size_t n_nodes, double *out, size_t out_doubles);
size_t rs_deal_trainer_br_bytes(const rs_deal_trainer *trainer);
int rs_deal_trainer_br_release(rs_deal_trainer *trainer);
int rs_deal_trainer_br_launches(const rs_deal_trainer *trainer, int sorted);
const uint8_t *rs_deal_trainer_cards(const rs_deal_trainer *trainer);  /* device: the current batch's d_cards[9][pitch] */
const float *rs_deal_trainer_signs(const rs_deal_trainer *trainer);    /* device: its showdown signs [pitch] */
const uint8_t *rs_deal_trainer_prune_flags(const rs_deal_trainer *trainer);   /* device: its per-deal prune flags [pitch] (all 0 before the threshold) */
const uint32_t *rs_deal_trainer_clusters(const rs_deal_trainer *trainer, int round_idx, int player);   /* device: its cluster ids [pitch] */

/* ---- abstraction generator's distance sweep: gen_abstraction/kmeans.rs, emd.rs -----------------------------
 * The sweep that WRITES the bucket files read above: Kmeans::predict over every canonical hand's histogram (main.rs:361-380).
 * Histograms are f32[n_bins] (type Histogram = Vec<f32>), 1..64 bins.  Arithmetic is the reference's, bit for bit: f32, no FMA, the
 * operation order of emd_1d (emd.rs:53-113) / l2_dist (kmeans.rs:622-630). */
enum { RS_DIST_EMD = 0,   /* emd::emd_1d */
       RS_DIST_L2 = 1 };  /* kmeans::l2_dist */
/* one dist_func(p, q) on the host */
int rs_histogram_distance(int dist, const float *p, const float *q, int n_bins, float *out);
/* Kmeans::predict (kmeans.rs:173-211): d_dataset = DEVICE [n][n_bins] row-major, centers = HOST [n_centers][n_bins];
 * d_clusters[n] (u32: first center with the strictly smallest distance) and d_min_dist[n] (that distance) are DEVICE buffers, either may
 * be NULL.  The reference's returned `inertia` is a racy load+store (kmeans.rs:205); sum d_min_dist instead.  Asynchronous on the table's
 * stream; `table` only lends its device and stream. */
int rs_kmeans_predict(rs_table *table, int dist, const float *d_dataset, size_t n, const float *centers, int n_centers, int n_bins,
                      uint32_t *d_clusters, float *d_min_dist);
/* update_min_dists (kmeans.rs:603-619), the kmeans++ step: d_min_dists[i] = min(d_min_dists[i], dist(dataset[i], new_center)^2) */
int rs_update_min_dists(rs_table *table, int dist, float *d_min_dists, const float *d_dataset, size_t n, const float *new_center, int n_bins);

/* The training loops that produce the centers (kmeans.rs:213-601), Hamerly-bounded: d_clusters (u32 [n]) and d_bounds (float [n][2] = (lower, upper) per datum) are
 * DEVICE arrays; centers and s live on the HOST; every f32 sum runs in the reference's order (means are summed in data order), so results are bit-identical to the
 * sequential Rust loops (rayon only ever parallelises loops whose iterations write their own element).  All of them synchronise.
 *   rs_kmeans_init_s        Kmeans::init_s (:267-285): s[i] = min(s[i], min_{j != i} dist(c_i, c_j)) / 2 -- s is IN/OUT, as coded (created once, :518)
 *   rs_kmeans_reassign      Kmeans::reassign_clusters (:287-334) = assignment_with_bounds (:213-265); d_order (may be NULL): datum i = dataset[d_order[i]]
 *   rs_kmeans_fit_regular   Kmeans::fit_regular (:497-600), `iterations` = 10 in the reference; centers in/out, d_clusters out, d_bounds / inertia out (may be NULL)
 *   rs_kmeans_fit_growbatch Kmeans::fit_growbatch AS CODED (:336-495: one pass over the first `batch` shuffled items, then `break`); the shuffle (:352) is the
 *                           caller's: d_order; stats (may be NULL) = {min_change, inertia as printed}
 * Limits of the two fits, refused (RS_ERR_UNSUPPORTED) before anything is launched or written -- d_clusters, d_bounds and centers are left as they were:
 *   at most 16 384 centers (rs_kmeans_fit_regular and rs_kmeans_fit_growbatch: one LDS counter per cluster in the member lists);
 *   at most 63 bins for rs_kmeans_fit_growbatch (one lane of a wave per bin, and one for the row of upper bounds); rs_kmeans_fit_regular takes 1..64.
 * Inputs of the whole family (the distances, predict, update_min_dists and the loops): finite, non-negative bins with a finite f32 sum.  emd_1d casts
 * round(n_bins / factor) to an integer, which has no defined value for NaN, so there is no contract for non-finite bins or rows whose f32 sum overflows. */
int rs_kmeans_init_s(rs_table *table, int dist, const float *centers, int n_centers, int n_bins, float *s);
/* Kmeans::init_random's choice among restarts (kmeans.rs:104-165): the caller draws the candidate center sets with its rng (`choose_multiple`, :120), this scores them
 * as coded (mean pairwise distance, f32 sums in index order, :133-148) and returns the most spread one (*best; the last of equal maxima, :151-156).
 * centers: HOST [n_restarts][n_centers][n_bins]; cluster_dists: HOST out [n_restarts], may be NULL.  (init_pp's heavy step is rs_update_min_dists.) */
int rs_kmeans_pick_restart(rs_table *table, int dist, const float *centers, int n_restarts, int n_centers, int n_bins, float *cluster_dists, int *best);
int rs_kmeans_reassign(rs_table *table, int dist, const float *d_dataset, const uint32_t *d_order, size_t n, const float *centers, int n_centers, int n_bins,
                       const float *s, uint32_t *d_clusters, float *d_bounds);
int rs_kmeans_fit_regular(rs_table *table, int dist, const float *d_dataset, size_t n, float *centers, int n_centers, int n_bins, int iterations, uint32_t *d_clusters,
                          float *d_bounds, float *inertia);
int rs_kmeans_fit_growbatch(rs_table *table, int dist, const float *d_dataset, size_t n, const uint32_t *d_order, size_t batch, float *centers, int n_centers,
                            int n_bins, uint32_t *d_clusters, float *d_bounds, float *stats);

/* ---- exact expected hand strength and the EHS histograms the k-means above clusters (gen_abstraction/ehs.rs, bin/gen_ehs.rs, main.rs generate_histograms) -------------
 * The reference samples (`calc_equity`, an unseeded SmallRng); here every run-out and every opponent hand is enumerated, so a result depends on the cards alone.
 * Cards are 4 * rank + suit.  A hand is two hole cards followed by 3, 4 or 5 board cards.  An opponent hand is any two of the remaining cards, each counted once.  A
 * completion is any SET of further board cards, drawn from what is left, that brings the board to 5 (unordered sets give the distribution of the reference's ordered draws).
 *   river, 7 cards   over the N = 990 opponent hands, W have a lower `evaluate` score and T an equal one: ehs = (float)((double)(2 W + T) / (double)(2 N)).
 *   flop / turn      the same formula with W, T and N summed over the completions: 1081 of a flop hand (N = 1081 * 990), 46 of a turn hand (N = 46 * 990) -- what
 *                    calc_equity(hand vs random, board) estimates.
 *   bin              rs_ehs_bin(value, n_bins) is get_bin (main.rs:58-70) literally: f32 interval = 1 / bins, threshold = 1 - interval, `threshold -= interval` in f32 going
 *                    down, a strict `>`.  The accumulated thresholds are NOT j / bins (at 20 bins the tenth is 0.49999988, so an exact 0.5 lands in bin 10; 0.95f in bin
 *                    18).  The thresholds are computed once on the host by that loop; the kernels take the same array.
 *   histogram        of a flop or turn hand: for each completion the river ehs of the 7 cards, count[rs_ehs_bin(ehs, n_bins)] += 1; out[k] = (float)count[k] /
 *                    (float)n_completions.
 * Everything before the last division is an integer: the results do not depend on the order of summation, the kernel form or the grouping. */
#define RS_EHS_MAX_BINS 64   /* the k-means' limit; the reference uses 20, 30 and 35 */
/* host only; RS_ERR_INVALID (negative) unless 1 <= n_bins <= RS_EHS_MAX_BINS */
int rs_ehs_bin(float value, int n_bins);
/* EHS::get_ehs for a list of hands, by enumeration: d_cards[n_cards][pitch] (u8, row i = card i of the hand, pitch = round_up(n, 64): the layout of
 * rs_hand_index_device), n_cards = 5, 6 or 7, d_out[n].  A plain per-hand kernel (a wave per 7-card hand, a workgroup per 5- or 6-card hand); it is the device-side
 * definition the sweep below is tested against.  RS_ERR_INVALID before anything is launched or allocated: n_cards not 5, 6 or 7, NULL d_cards or d_out with n > 0.
 * A hand with a repeated card or a byte >= 52 raises an error word that THIS call reads back: it synchronises and returns RS_ERR_INVALID; the outputs of such hands
 * are left as they were, every other hand's is written. */
int rs_ehs(rs_table *table, const uint8_t *d_cards, int n_cards, uint32_t n, float *d_out);
/* The histograms of a whole round.  `indexer` = hand_indexer_s::init(2, [2, 3]) (flop) or (2, [2, 4]) (turn); d_out[rs_hand_indexer_size(indexer, 1)][n_bins].
 * d_boards[3 or 4][pitch] (pitch = round_up(n_boards, 64)) lists boards; NULL = every board of the round (22 100 flops / 270 725 turn boards, enumerated on the device;
 * n_boards is ignored).  For each board the histogram of every hole pair that fits it (1176 on a flop, 1128 on a turn board) is written to the row of the hand's canonical
 * index; rows whose hands lie on no listed board are left as they were.  Suit-isomorphic copies of a hand (on one board or on several) write IDENTICAL BITS to the same
 * row -- the integer counts are equal and the one division is the same -- and this is relied on: the writes are plain stores, unordered.
 * RS_ERR_INVALID before anything is launched or allocated: an indexer of another shape, n_bins outside 1..RS_EHS_MAX_BINS, NULL d_out with boards to do.  A listed board
 * with a repeated card or a byte >= 52 is skipped and reported as for rs_ehs (error word read back by this call, RS_ERR_INVALID; the other boards' rows are written).
 * Synchronises. */
int rs_ehs_round_histograms(rs_table *table, rs_hand_indexer *indexer, int n_bins, const uint8_t *d_boards, uint32_t n_boards, float *d_out);

/* ---- exact OCHS features: a hand's equity against each of a few opponent ranges (gen_abstraction/main.rs:161-330 gen_ochs) ---------------------------------------------
 * The river's bucket file comes from an L2 k-means over these vectors (a river hand has one EHS value, not a distribution).  The reference samples them
 * (`calc_equity(..., 1000)`, thread_rng) and ships the generator commented out; here, as above, everything is enumerated.
 *   opponent partition   pair_cluster[1326] (host): one entry per hole pair c0 < c1 at index c1 (c1 - 1) / 2 + c0, a cluster id 0 .. n_clusters - 1 or
 *                        RS_OCHS_NO_CLUSTER for a hand that is in no range; 1 <= n_clusters <= RS_OCHS_MAX_CLUSTERS (the reference's n_opp_clusters is 8).  Any
 *                        partition is taken: nothing here knows of preflop classes.
 *   feature of a hand    hole pair h and a board b of 3, 4 or 5 cards.  For cluster k, over every completion r of the board to 5 cards from the cards not in h or b
 *                        (the river has the single empty one) and every opponent pair o with pair_cluster[o] == k that shares no card with h, b or r: W_k score lower
 *                        than h, T_k equal, N_k is their count.  e_k = (float)((double)(2 W_k + T_k) / (double)(2 N_k)), and +0.0 where N_k == 0.
 *   normalize != 0       the reference's hist[i] /= norm_sum (main.rs:281-297): s = e_0 + e_1 + ... in f32 in index order, out_k = e_k / s in f32.  A row whose s is 0
 *                        stays all +0.0 (the reference would write NaN there).
 *   preflop counts       for hole pair p and a flop f that shares no card with it, count_f[p][bin] = the number of the 1081 completions whose river EHS (rs_ehs's
 *                        value) falls in rs_ehs_bin(., n_bins): the un-normalised row of rs_ehs_round_histograms.  counts[p][bin] sums them over the swept flops.  Over
 *                        all 22 100 flops each of the pair's C(50, 5) boards is met C(5, 3) = 10 times: every row sums to 21 187 600, every cell is a multiple of 10.
 * Everything before the last division is an integer (2 W + T <= 2 * 1176 * 990): nothing depends on summation order or kernel form. */
#define RS_OCHS_MAX_CLUSTERS 8
#define RS_OCHS_NO_CLUSTER   255
/* indexer = hand_indexer_s::init(2, [2, 3] | [2, 4] | [2, 5]); d_out[rs_hand_indexer_size(indexer, 1)][n_clusters].
 * d_boards[3|4|5][pitch] (pitch = round_up(n_boards, 64)) lists boards (any order of cards within a board): the rows of the 1176 / 1128 / 1081 hole pairs of each are
 * written, the others left as they were.  NULL = the whole round: every row of d_out is written, with the bits that listing all C(52, nb) boards would give (the call
 * sweeps one board per suit-isomorphism class -- 1 755 / 16 432 / 134 459 -- from a list it builds, uploads and frees).  Suit-isomorphic copies write identical bits:
 * plain stores.  RS_ERR_INVALID before anything is launched or allocated: an indexer of another shape, n_clusters out of range, a pair_cluster entry that is neither
 * an id below n_clusters nor RS_OCHS_NO_CLUSTER, NULL d_out with work to do.  A listed board with a repeated card or a byte >= 52 is skipped and reported as for
 * rs_ehs_round_histograms (RS_ERR_INVALID, the other boards done).  Synchronises. */
int rs_ochs_round_features(rs_table *table, rs_hand_indexer *indexer, const uint8_t *pair_cluster, int n_clusters, int normalize,
                           const uint8_t *d_boards, uint32_t n_boards, float *d_out);
/* d_counts[1326][n_bins] uint32 (row = c1 (c1 - 1) / 2 + c0), zeroed by the call; d_boards[3][pitch] or NULL = all 22 100 flops.  RS_ERR_INVALID before anything is
 * launched or allocated: n_bins outside 1..RS_EHS_MAX_BINS, NULL d_counts.  A bad listed board: as above.  Synchronises. */
int rs_ehs_preflop_counts(rs_table *table, int n_bins, const uint8_t *d_boards, uint32_t n_boards, uint32_t *d_counts);

/* ---- potential-aware abstraction: next-round bucket histograms and a k-means under the greedy earth mover's distance (rs_potential.hip) ---------------------------------
 * Ganzfried and Sandholm, "Potential-aware imperfect-recall abstraction with earth mover's distance in imperfect-information games" (AAAI 2014); DESIGN.md section 4.
 *   row of a hand      hole pair + a board of nb = 3 or 4 cards; n_draws = 50 - nb.  For every card x in neither, bucket(x) = next_buckets[hand_index of
 *                      (hole, board + x) in the next round's indexer [2, nb + 1]].  The row is the multiset of those buckets: uint32 row[RS_PA_ROW_WORDS], entries
 *                      `bucket << 8 | count` with count >= 1, ascending by bucket, then zeros.  The counts sum to n_draws.  A WELL-FORMED row is exactly that: m >= 1
 *                      entries with strictly ascending buckets below n_next and counts >= 1 that sum to n_draws, followed by RS_PA_ROW_WORDS - m zero words.
 *   metric             ground[n_next][n_next] (finite, >= 0): ground[b][t] is what moving mass from bucket b of a point to bucket t of a mean costs.
 *                      order[b][.] = the ids 0 .. n_next - 1 sorted stably by ascending ground[b][.] (among equal distances the lower id first).
 *   distance           of a row p with entries (b_j, c_j), j = 0 .. m - 1, to a dense mean q[n_next] (finite, >= 0) -- the paper's Algorithm 2 in f32 without FMA:
 *                          rem = copy of q;  target[j] = (float)c_j / (float)n_draws;  tot[j] = 0;  done[j] = false
 *                          for i = 0 .. n_next - 1, for j = 0 .. m - 1 ascending, unless done[j]:
 *                              t = order[b_j][i];  a = rem[t];  unless a > 0: next j;  d = ground[b_j][t]
 *                              a < target[j]:  tot[j] += a * d;  target[j] -= a;  rem[t] = 0
 *                              otherwise:      tot[j] += target[j] * d;  rem[t] = a - target[j];  target[j] = 0;  done[j] = true
 *                          dist = ((0.0f + tot[0]) + tot[1]) + ... + tot[m - 1]
 *                      The per-entry totals summed in entry order are this library's choice (the paper keeps one running total).  Neither symmetric nor a metric.
 *                      `a > 0` is the IEEE f32 comparison, on the device as on the host: a subnormal is positive and is taken from, -0.0 is not; nothing is flushed to
 *                      zero.  A total may overflow to +inf (never to NaN: no ground entry is infinite); among means at +inf the first is chosen, as among any equals.
 *   k-means            assignment = the first mean with the strictly smallest distance (rs_kmeans_predict's rule).  One Lloyd iteration: assign every datum;
 *                      changed = the data whose cluster differs from the iteration before (before the first: none, so changed[0] = n); for every cluster k with
 *                      members: mean[k][b] = (float)((double)sum[k][b] / ((double)members[k] * (double)n_draws)), sum = the integer sum of its members' counts; a
 *                      cluster without members keeps its mean; the loop stops after an iteration with changed == 0. */
#define RS_PA_ROW_WORDS 48
#define RS_PA_MAX_NEXT 8192
typedef struct rs_pa_metric rs_pa_metric;
/* indexer = hand_indexer_s::init(2, [2, 3] | [2, 4]), next_indexer = (2, [2, 4] | [2, 5]); d_next_buckets: DEVICE uint32 [rs_hand_indexer_size(next_indexer, 1)];
 * d_rows: DEVICE uint32 [rs_hand_indexer_size(indexer, 1)][RS_PA_ROW_WORDS].  d_boards[nb][pitch] (pitch = round_up(n_boards, 64)) lists boards: the rows of their hole
 * pairs are written, the others left as they were.  NULL = the whole round, swept as one board per suit-isomorphism class: every row is written.  Suit-isomorphic copies of
 * a hand write identical bits: plain stores.  RS_ERR_INVALID before anything is launched: indexers of any other shape pair, n_next outside 1..RS_PA_MAX_NEXT, NULL buffers
 * with work to do.  A listed board with a repeated card or a byte >= 52 is skipped, and so is a hand one of whose buckets is >= n_next; either raises an error word that this
 * call reads back: RS_ERR_INVALID, everything else written.  Synchronises. */
int rs_next_round_histograms(rs_table *table, rs_hand_indexer *indexer, rs_hand_indexer *next_indexer, const uint32_t *d_next_buckets, int n_next,
                             const uint8_t *d_boards, uint32_t n_boards, uint32_t *d_rows);
/* ground: HOST [n_next][n_next], 1 <= n_next <= RS_PA_MAX_NEXT; a value that is negative or not finite is RS_ERR_INVALID.  `order` is built here, once, and both are
 * uploaded to the table's device.  table == NULL gives a host-only metric: rs_pa_distance takes it, the device calls refuse it. */
int rs_pa_metric_create(rs_table *table, const float *ground, int n_next, rs_pa_metric **out);
void rs_pa_metric_destroy(rs_pa_metric *metric);
/* one distance on the host (no GPU needed).  RS_ERR_INVALID: a row that is not well-formed, a mean value that is negative or not finite */
int rs_pa_distance(const rs_pa_metric *metric, const uint32_t *row /* HOST [RS_PA_ROW_WORDS] */, int n_draws, const float *mean /* HOST [n_next] */, float *out);
/* d_rows: DEVICE [.][RS_PA_ROW_WORDS]; datum i is row d_sel[i] (d_sel == NULL: row i); means: HOST [n_means][n_next]; d_clusters[n] / d_min_dist[n]: DEVICE, either may
 * be NULL.  A row that is not well-formed raises the error word: its outputs are left as they were and the call returns RS_ERR_INVALID after the others are done.
 * Both synchronise.  rs_pa_fit: means in/out, changed: HOST [iterations], iterations_run (may be NULL) = the iterations done; d_clusters and d_min_dist are those of the
 * last assignment (a datum whose row is not well-formed belongs to no cluster: d_clusters = 0xFFFFFFFF). */
int rs_pa_predict(rs_table *table, const rs_pa_metric *metric, const uint32_t *d_rows, const uint32_t *d_sel, size_t n, int n_draws, const float *means, int n_means,
                  uint32_t *d_clusters, float *d_min_dist);
int rs_pa_fit(rs_table *table, const rs_pa_metric *metric, const uint32_t *d_rows, const uint32_t *d_sel, size_t n, int n_draws, float *means, int n_means, int iterations,
              uint32_t *d_clusters, float *d_min_dist, uint32_t *changed, int *iterations_run);

/* ---- showdown evaluation on the device ---------------------------------------------------------------
 * d_cards[9][pitch] (u8, pitch = round_up(n_deals, 64)): rows 0-4 the board, 5-6 player 0's hole cards, 7-8 player 1's;
 * card = 4*rank + suit, rank 0..12 = 2..A (cfr.rs:592).  d_sign[lane] = sign(evaluate(hand0) - evaluate(hand1)) exactly as
 * cfr.rs:324-333 compares the two scores: ready to be used as an RS_LEAF_SIGN buffer. */
int rs_showdown_sign(rs_table *table, const uint8_t *d_cards, uint32_t n_deals, float *d_sign);

/* ---- table checkpoints (the reference never persists the trained table) ----------------------------
 * "RSTB" v1: header, node descriptors, then per node regrets[A][lanes] and strategy_sum[A][lanes] (no pitch padding),
 * then a 64-bit FNV-1a checksum.  rs_table_load creates the table on `device`. */
int rs_table_save(rs_table *table, const char *path);
int rs_table_load(const char *path, int device, rs_table **out);

/* ---- multi-GPU: boards shard across GPUs, one process per GPU -------------------------
 * Replicated tables (rounds whose boards are not sharded) accumulate rank-local deltas; one RCCL
 * all-reduce (sum) over xGMI brings every rank to the same values. */
#define RS_COMM_ID_BYTES 128
int rs_comm_unique_id(void *id_out /* RS_COMM_ID_BYTES */);   /* rank 0; ship the bytes to the other ranks */
int rs_comm_create(rs_table *table, const void *id, int rank, int n_ranks, rs_comm **out);
void rs_comm_destroy(rs_comm *comm);
/* snapshot the replicated rounds (bit r of round_mask) before a local iteration ... */
int rs_replicated_begin(rs_table *table, uint32_t round_mask);
/* ... then x = snapshot + allreduce_sum(x - snapshot) for regrets and strategy_sum of those rounds */
int rs_allreduce_replicated(rs_table *table, rs_comm *comm, uint32_t round_mask);

#ifdef __cplusplus
}
#endif
#endif /* RUSTSOLVER_AMD_H */
