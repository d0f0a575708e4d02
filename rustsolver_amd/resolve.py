"""Safe subgame re-solving: the recipe of DESIGN.md section 5e as code.

    prepared = resolve.prepare(trunk_table, trunk_tree, board0, hands, clusters, node, prefix, resolver)
    sub_table = create_infosets(prepared.tree.n_action_nodes, prepared.tree, sizes[prepared.round0:], [1] * len(prepared.clusters), dtype=F32)
    solver = RangeCFR(sub_table, prepared.tree, prepared.board, prepared.hands[0], prepared.hands[1], prepared.clusters, weights=prepared.weights, deal="joint")
    solver.set_gadget(prepared.resolver, prepared.alt)
    solver.train(...)
    resolve.graft(sub_table, trunk_table, prepared, prepared.resolver)

prepare cuts the subtree below `node` (GameTree.subtree), asks the node report for both players' rows at the node and reads row `prefix` (the board of the node's round
the subgame is played on), and turns them into the inputs of a full-width solver with the re-solving gadget (Burch, Johanson, Bowling 2014) above the root:
  * the resolver's range weights are its own reach times its prior; hands of weight 0 leave the range;
  * the opponent's weights are its prior ALONE -- the gadget has to be safe against every hand the opponent may hold, so the opponent's trunk reach is not applied --
    and only hands that share a card with the prefix's board leave the range;
  * alt[h] = value / mass of the opponent's row: what hand h is worth in the trunk per unit of the resolver's reach mass it faces (0.0 where the mass is 0);
  * the cluster tables of the rounds from the node's on are the trunk's rows under the prefix (the run-outs of the longer board are enumerated in the trunk's order under
    that prefix), ids kept: a table created with the trunk's cluster counts of those rounds accepts them.
The trunk's deal distribution is handed in as `weights` / `deal` where it is not the default.  The conditional distribution at the node is exactly the subgame's "joint"
deal when the trunk's is of product form (a "joint" trunk); for a "sequential" trunk the difference belongs into `prior`.
"""
from collections import namedtuple

import numpy as np

from . import _lib as L
from .solver import drop_zero_weights

Prepared = namedtuple("Prepared", "tree node_map index_map board hands clusters weights alt resolver round0 keep foreign")
Prepared.__doc__ = """tree, node_map: GameTree.subtree(node); index_map[k] = the trunk's action index of the subtree's action index k; board: the 4- or 5-card board;
hands[p], clusters[r][p], weights[p]: the kept hands, their columns of the sliced cluster tables (round r counted from the node's round round0) and their range weights;
alt: one value per kept hand of the opponent; keep[p]: bool mask over the trunk's hands; foreign[r][p]: the cluster ids that occur under the OTHER prefixes of the round"""


def prepare(table, tree, board0, hands, clusters, node, prefix, resolver, current=False, prior=(None, None), weights=None, deal="sequential", sorted_showdowns=True):
    if resolver not in (0, 1):
        raise ValueError("resolver is 0 or 1")
    P, O = int(resolver), 1 - int(resolver)
    board0 = [int(c) for c in np.asarray(board0).reshape(-1)]
    hands = [np.ascontiguousarray(h, dtype=np.uint8).reshape(-1, 2) for h in hands]
    sub, node_map = tree.subtree(node)                                             # refuses anything but an action node
    r0 = int(tree.nodes[int(node)].round_idx)
    K, D = 5 - len(board0), 52 - len(board0)
    n_prefixes = [int(np.prod([D - i for i in range(r)], dtype=np.int64)) for r in range(K + 1)]
    if r0 > K or not (0 <= prefix < n_prefixes[r0]):
        raise ValueError("prefix %d: round %d of this game has %d prefixes" % (prefix, r0, n_prefixes[min(r0, K)]))
    # the prefix's new cards: the first new card most significant, cards ascending among those still in the deck
    board, rest = list(board0), int(prefix)
    for i in range(r0):
        deck = [c for c in range(52) if c not in board]
        per = n_prefixes[r0] // int(np.prod([D - j for j in range(i + 1)], dtype=np.int64))
        board.append(deck[rest // per])
        rest %= per
    rep = [table.node_report(tree, board0, hands[0], hands[1], clusters, p, [int(node)], current=current, sorted_showdowns=sorted_showdowns, weights=weights,
                             deal=deal)[int(node)] for p in (0, 1)]
    pr = [np.ones(len(hands[p])) if prior[p] is None else np.asarray(prior[p], dtype=np.float64).reshape(-1) for p in (0, 1)]
    w = [None, None]
    w[P] = rep[P]["own"][prefix] * pr[P]
    w[O] = np.where((hands[O][:, :, None] == np.array(board)[None, None, :]).any(axis=(1, 2)), 0.0, pr[O])
    value, mass = rep[O]["value"][prefix], rep[O]["mass"][prefix]
    alt = np.where(mass > 0, value / np.where(mass > 0, mass, 1.0), 0.0)
    sliced, foreign = [], []
    for r in range(r0, len(clusters)):
        k = n_prefixes[r] // n_prefixes[r0]                                         # prefixes of round r under one prefix of round r0
        rows, other = [], []
        for p in (0, 1):
            c = np.asarray(clusters[r][p], dtype=np.uint32).reshape(-1, len(hands[p]))
            mine = np.zeros(len(c), dtype=bool)
            mine[prefix * k:(prefix + 1) * k] = True
            rows.append(c[mine])
            other.append(np.unique(c[~mine]))
        sliced.append(rows)
        foreign.append(other)
    kept_hands, kept_clusters, kept_w, keep = drop_zero_weights(hands, sliced, w)
    index_map = np.full(sub.n_action_nodes, -1, dtype=np.int64)
    for i, nd in enumerate(sub.nodes):
        if nd.kind == L.NODE_ACTION:
            index_map[nd.index] = tree.nodes[int(node_map[i])].index
    return Prepared(sub, node_map, index_map, np.array(board, dtype=np.uint8), kept_hands, kept_clusters, kept_w, np.ascontiguousarray(alt[keep[O]]), P, r0, keep, foreign)


def trunk_rows(trunk_table, prepared):
    """a new F32 table of the subtree's action nodes holding the trunk's rows (regrets and strategy sums) of those nodes, through index_map: the trunk's profile as a
    profile of the subgame, to be READ (best_response_alt, margins, a node report), not trained on -- the cells of an I32 trunk are copied as numbers, without their
    integer scale, which the strategies read from them do not depend on"""
    from .solver import InfosetTable
    descs, rows = [], []
    for t in prepared.index_map:
        d = trunk_table.node_desc(int(t))
        descs.append((d.n_actions, d.n_clusters, d.n_boards, d.player, d.round_idx - prepared.round0))
        rows.append(trunk_table.download_node(int(t)))
    sub = InfosetTable.create(descs, dtype=L.F32)
    for k, (R, S) in enumerate(rows):
        sub.upload_node(k, R.astype(np.float32), S.astype(np.float32))
    return sub


def _opponent_hands(sub_table, prepared, current):
    O = 1 - prepared.resolver
    return sub_table.best_response_hands(prepared.tree, prepared.board, prepared.hands[0], prepared.hands[1], prepared.clusters, O,
                                         mode=L.BR_MAX | L.BR_REAL | L.BR_SORTED, current=current, weights=prepared.weights, deal="joint")


def best_response_alt(sub_table, prepared, current=False):
    """the counterfactual best-response alt: per kept hand of the opponent, value / mass of its best response in the real game (best_response_hands, BR_MAX | BR_REAL |
    BR_SORTED) against sub_table's profile on the subgame's weights; 0.0 where the mass is 0.  With sub_table = trunk_rows(...) this is the alternative value both
    re-solving papers assume; prepared.alt is the value under the trunk profile itself."""
    value, mass = _opponent_hands(sub_table, prepared, current)
    return np.where(mass > 0, value / np.where(mass > 0, mass, 1.0), 0.0)


def margins(sub_table, prepared, alt=None, current=False):
    """the check of a re-solve: alt - value / mass per kept hand of the opponent, value / mass its best-response value against sub_table's profile (as best_response_alt);
    a re-solve is safe for a hand whose margin is >= 0.  alt=None: prepared.alt.  NaN where the mass is 0."""
    alt = prepared.alt if alt is None else np.asarray(alt, dtype=np.float64).reshape(-1)
    value, mass = _opponent_hands(sub_table, prepared, current)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(mass > 0, alt - value / np.where(mass > 0, mass, 1.0), np.nan)


def graft(sub_table, trunk_table, prepared, player):
    """copies the player's re-solved rows (regrets and strategy sums) of the subtree's nodes back into the trunk table, for the cluster ids that occur under the prefix"""
    todo = []
    for nd in prepared.tree.action_nodes():
        if nd.player != player:
            continue
        ids = np.unique(prepared.clusters[nd.round_idx][player])
        if np.intersect1d(ids, prepared.foreign[nd.round_idx][player]).size:
            raise ValueError("cluster ids of the subgame also occur under another prefix of the same round: the abstraction shares these cells across boards, "
                             "so grafting would rewrite the strategy on other boards")
        todo.append((nd.index, ids))
    for k, ids in todo:                                                             # every check has passed: only now is the trunk written
        t = int(prepared.index_map[k])
        R, S = trunk_table.download_node(t)
        Rs, Ss = sub_table.download_node(k)
        R[:, ids], S[:, ids] = Rs[:, ids], Ss[:, ids]
        trunk_table.upload_node(t, R, S)
