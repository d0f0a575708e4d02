"""CPU: safe subgame re-solving restated in numpy (tests/np_resolve.py) against what the construction is known to do.  No device, no library.

  a. the subtree cut on both golden trees: node counts, index renumbering, rebased rounds, unchanged terminals; a cut at the root is the identity;
  b. the units of the recipe: under the trunk's own profile FOLLOW is worth exactly the alternative, for every opponent hand (alt units, cluster slicing, run-out order);
  c. a gadget that always follows is no gadget: the resolver's sweep is np_range_cfr.sweep bit for bit;
  d. safety: grafting a gadget re-solve does not raise the opponent's best-response value (the numbers are in the test's docstring);
  e. two summation orders of one gadget sweep stay within test_range_cfr_cpu.compare_cells' rule on the cases tests/test_gpu_resolve.py runs: what entitles that
     file to the rule.
The GPU file imports CASES, gadget_inputs, order_check and the safety game from here."""
import json
import os

import numpy as np
import pytest

import np_node_report as nnr
import np_range_cfr as nrc
import np_resolve as nr
import np_weighted as nw
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_gpu_range_cfr import make_case
from test_np_br_cpu import ATOL, TURN, lane_cids, pick_ranges, random_cids, sizes_of
from test_range_cfr_cpu import TURN_TREE, compare_cells, random_tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THREE_STREET = dict(n_board_cards=3, bet_sizes=((0.5, 1.0),) * 3, raise_sizes=((3.0,),) * 3)


def golden_trees():
    """the river tree as stored; the three-street tree rebuilt from its options and held against the stored summary"""
    river = json.load(open(os.path.join(GOLDEN, "tree_river.json")))["nodes"]
    fx = json.load(open(os.path.join(GOLDEN, "tree_three_street.json")))
    three, n_act = npr.build_tree(**THREE_STREET)
    assert (len(three), n_act) == (fx["n_nodes"], fx["n_action_nodes"])
    assert [[d["index"], d["player"], d["round_idx"], len(d["children"])] for d in three if d["kind"] == "action"] == fx["action_nodes"]
    return {"river": river, "three_street": three}


def descendants(nodes):
    """per node: the number of nodes below it (children come after their parents)"""
    below = [0] * len(nodes)
    for i in range(len(nodes) - 1, 0, -1):
        below[nodes[i]["parent"]] += below[i] + 1
    return below


# ---- a ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["river", "three_street"])
def test_subtree_cut_on_the_golden_trees(name):
    nodes = golden_trees()[name]
    below = descendants(nodes)
    for node, root in enumerate(nodes):
        if root["kind"] != "action":
            with pytest.raises(ValueError):
                nr.cut(nodes, node)
            continue
        sub, node_map = nr.cut(nodes, node)
        assert len(sub) == below[node] + 1 == len(node_map) and node_map[0] == node and sub[0]["parent"] == -1
        assert (np.diff(node_map) > 0).all()                                       # the trunk's relative order
        acts = [(nd["index"], nodes[int(t)]["index"]) for nd, t in zip(sub, node_map) if nd["kind"] == "action"]
        assert sorted(a for a, _ in acts) == list(range(len(acts)))                # a permutation ...
        assert [t for _, t in sorted(acts)] == sorted(t for _, t in acts)          # ... ascending in the trunk's index
        for i, (nd, t) in enumerate(zip(sub, node_map)):
            old = nodes[int(t)]
            assert nd["kind"] == old["kind"] and [int(node_map[c]) for c in nd["children"]] == old["children"]
            assert i == 0 or int(node_map[nd["parent"]]) == old["parent"]
            if nd["kind"] == "action":
                assert nd["round_idx"] == old["round_idx"] - root["round_idx"] and nd["player"] == old["player"] and nd["actions"] == old["actions"]
            elif nd["kind"] == "terminal":
                assert all(nd[k] == old[k] for k in ("value", "ttype", "last_to_act", "round"))
            elif "round" in old:
                assert nd["round"] == old["round"]
        assert (nr.index_map(nodes, sub, node_map) == [t for _, t in sorted(acts)]).all()
    first = next(i for i, nd in enumerate(nodes) if nd["kind"] == "action")
    sub, node_map = nr.cut(nodes, first)                                           # the root action node: everything but the chance node above it, numbered as it was
    assert (node_map == np.arange(first, len(nodes))).all()
    assert all(nd["kind"] != "action" or (nd["index"], nd["round_idx"]) == (nodes[int(t)]["index"], nodes[int(t)]["round_idx"]) for nd, t in zip(sub, node_map))
    if name == "river":                                                            # ... and at a tree whose root IS the action node the cut is the identity
        again, m2 = nr.cut(sub, 0)
        assert again == sub and (m2 == np.arange(len(sub))).all()


# ---- b ---------------------------------------------------------------------------------------------------------------------------------------------------------
def turn_trunk():
    """the turn-start game of test_range_cfr_cpu (9 x 7 hands, one info set per lane), a JOINT trunk with unit weights -- product form, so the conditional distribution
    at a node is exactly the subgame's -- and random f32 regrets"""
    rng = np.random.Generator(np.random.PCG64(7))
    h = pick_ranges(rng, TURN, 9, 7)
    cids = lane_cids(TURN, h)
    sizes = sizes_of(cids)
    nodes, _ = npr.build_tree(n_board_cards=4, bet_sizes=TURN_TREE[0], raise_sizes=TURN_TREE[1])
    tables = random_tables(np.random.Generator(np.random.PCG64(3)), nodes, sizes)
    return nodes, h, cids, sizes, nw.WeightedGame(TURN, h, (None, None), "joint"), tables


def test_the_runouts_of_the_longer_board_are_the_trunks_order_under_the_prefix():
    trunk = nbr.runouts(TURN)
    for prefix in range(48):
        assert (nbr.runouts([int(c) for c in trunk[prefix][:5]]) == trunk[prefix:prefix + 1]).all()
    flop = nbr.runouts(TURN[:3])
    for prefix in (0, 11, 48):
        assert (nbr.runouts([int(c) for c in flop[prefix * 48][:4]]) == flop[prefix * 48:(prefix + 1) * 48]).all()


@pytest.mark.parametrize("round0", [0, 1])
def test_follow_under_the_trunks_own_profile_is_worth_the_alternative(round0):
    """prepare(current=True) at turn-round and river-round nodes, the trunk's regret rows copied into the subgame through the index map, one gadget sweep of the opponent
    from zero gadget rows: |S[1] - S[0]| <= 1e-9 * max|S[0]| for every opponent hand (the sums differ in f64 order only: 48 x 1 326 terms x 2^-53 is 7e-12 relative)"""
    nodes, h, cids, sizes, game, tables = turn_trunk()
    picked = [i for i, nd in enumerate(nodes) if nd["kind"] == "action" and nd["round_idx"] == round0]
    picked = [picked[0], picked[len(picked) // 2], picked[-1]]
    checked = 0
    for node in picked:
        for prefix in ([0] if round0 == 0 else [0, 5, 17, 47]):
            for P in (0, 1):
                pre = nr.prepare(nodes, tables, TURN, h, cids, node, prefix, P, current=True, game=game)
                assert len(pre["board"]) == 4 + round0 and len(pre["clusters"]) == 2 - round0
                sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
                R, S = nr.sub_tables(tables, pre)
                G = nr.new_gadget(P, pre["alt"])
                detail = {}
                nr.gadget_sweep(pre["nodes"], R, S, G, sub_game, pre["clusters"], 1 - P, detail=detail)
                bound = 1e-9 * np.abs(detail["S0"]).max()
                assert bound > 0 and (np.abs(detail["S1"] - detail["S0"]) <= bound).all(), (node, prefix, P, np.abs(detail["S1"] - detail["S0"]).max(), bound)
                assert (np.abs(G["regret"]) <= np.float32(bound)).all()            # ... so the gadget has nothing to regret
                checked += int(detail["used"].sum())
    assert checked > 30


def test_graft_refuses_cluster_ids_shared_across_boards():
    nodes, h, cids, sizes, game, tables = turn_trunk()
    shared = random_cids(np.random.Generator(np.random.PCG64(1)), TURN, h, [(3, 4), (5, 6)])
    tb = random_tables(np.random.Generator(np.random.PCG64(2)), nodes, [(3, 4), (5, 6)])
    river_node = next(i for i, nd in enumerate(nodes) if nd["kind"] == "action" and nd["round_idx"] == 1)
    pre = nr.prepare(nodes, tb, TURN, h, shared, river_node, 3, 0, game=game)
    kept = ({i: x.copy() for i, x in tb[0].items()}, {i: x.copy() for i, x in tb[1].items()})
    with pytest.raises(ValueError, match="shares these cells across boards"):
        nr.graft(nr.sub_tables(tb, pre), tb, pre, 0)
    assert all(tb[k][i].tobytes() == kept[k][i].tobytes() for k in (0, 1) for i in tb[k])
    pre = nr.prepare(nodes, tables, TURN, h, cids, river_node, 3, 0, game=game)     # one info set per lane: legal, and it writes only the prefix's cells
    sub = nr.sub_tables(tables, pre)
    for k in (0, 1):
        for i in sub[k]:
            sub[k][i] = sub[k][i] + np.float32(1.0)
    before = ({i: x.copy() for i, x in tables[0].items()}, {i: x.copy() for i, x in tables[1].items()})
    nr.graft(sub, tables, pre, 0)
    changed = sum(int((tables[k][i] != before[k][i]).sum()) for k in (0, 1) for i in tables[k])
    own = [nd for nd in pre["nodes"] if nd["kind"] == "action" and nd["player"] == 0]
    assert changed == 2 * sum(len(nd["children"]) for nd in own) * len(pre["hands"][0])


# ---- the cases of the GPU file -------------------------------------------------------------------------------------------------------------------------------------
CASES = ["river_lanes", "river_wave_35", "turn_lanes", "turn_imperfect_recall", "turn_one_hand", "turn_no_opponent"]


def gadget_inputs(rng, n, rows="random"):
    """alt with negative, zero and 1e30 entries; gadget rows drawn like random_tables' with every third hand's regrets non-positive (get_strategy's uniform branch),
    or zero rows"""
    alt = rng.standard_normal(n) * 20.0
    alt[1::5] = 0.0
    alt[3::5] = 1e30
    if n > 2:
        alt[2] = -abs(alt[2]) - 1.0
    if rows == "zero":
        return alt, np.zeros((2, n), dtype=np.float32), np.zeros((2, n), dtype=np.float32)
    regret = (rng.standard_normal((2, n)) * rng.choice([0.01, 1.0, 30.0], size=n)[None, :]).astype(np.float32)
    regret[:, 2::3] = -np.abs(regret[:, 2::3])
    if n > 5:
        regret[:, 5] = 0.0
    ssum = (rng.random((2, n)) * 10.0).astype(np.float32)
    return alt, regret, ssum


def copy_tables(R, S):
    return {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}


def order_check(name, nodes, cids, sizes, game, seed=51):
    """both resolvers, both traversers, plain and RM+, random and zero gadget rows: the reversed summation order against the restatement's own, cell by cell under
    compare_cells, the gadget's 4 n cells counted with the table's; -> (cells, cells that differ at all)"""
    cells = differ = 0
    for P in (0, 1):
        for p in (0, 1):
            for rmplus in (False, True):
                for rows in ("random", "zero"):
                    rng = np.random.Generator(np.random.PCG64(seed + 8 * P + 4 * p + 2 * rmplus + (rows == "zero")))
                    R, S = random_tables(rng, nodes, sizes)
                    alt, gr, gs = gadget_inputs(rng, game.n[1 - P], rows)
                    out = []
                    for reverse in (False, True):
                        Rk, Sk = copy_tables(R, S)
                        G = dict(resolver=P, alt=alt, regret=gr.copy(), ssum=gs.copy())
                        v = nr.gadget_sweep(nodes, Rk, Sk, G, game, cids, p, rmplus, reverse=reverse)
                        out.append((v, Rk, Sk, G))
                    (v1, R1, S1, G1), (v2, R2, S2, G2) = out
                    assert abs(v1 - v2) <= 1e-11 * abs(v1) + ATOL, (name, P, p, rmplus, rows, v1, v2)
                    pairs = [(R1[i], R2[i]) for i in R1] + [(S1[i], S2[i]) for i in S1] + [(G1["regret"], G2["regret"]), (G1["ssum"], G2["ssum"])]
                    for a, b in pairs:
                        d, _ = compare_cells(a, b, (name, P, p, rmplus, rows))
                        cells += d.size
                        differ += int((d > 0).sum())
    return cells, differ


# ---- c ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["river_lanes", "turn_imperfect_recall"])
def test_a_gadget_that_always_follows_is_no_gadget(name):
    """regret = (0, 1) gives sigma = (0, 1): the resolver's sweep writes the tables np_range_cfr.sweep writes on the same weighted game, bit for bit, value + 0.0"""
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    rng = np.random.Generator(np.random.PCG64(61))
    game = nw.WeightedGame(board0, h, (rng.random(len(h[0])) + 0.5, rng.random(len(h[1])) + 0.5), "joint")
    for P in (0, 1):
        for rmplus in (False, True):
            before = random_tables(rng, nodes, sizes)
            alt, _, gs = gadget_inputs(rng, game.n[1 - P])
            G = dict(resolver=P, alt=alt, regret=np.stack([np.zeros(game.n[1 - P]), np.ones(game.n[1 - P])]).astype(np.float32), ssum=gs.copy())
            got, want = copy_tables(*before), copy_tables(*before)
            v = nr.gadget_sweep(nodes, got[0], got[1], G, game, cids, P, rmplus)
            w = nrc.sweep(nodes, want[0], want[1], game, cids, P, rmplus)
            assert v == w
            assert all(got[k][i].tobytes() == want[k][i].tobytes() for k in (0, 1) for i in got[k])
            assert G["ssum"].tobytes() == gs.tobytes()                             # the resolver's sweep leaves the gadget rows


def test_a_sweep_touches_only_its_own_side():
    """the opponent's sweep leaves the resolver's rows, the resolver's sweep the gadget rows and the opponent's; hands without a dealt lane keep their gadget cells"""
    board0, h, cids, sizes, tree = make_case("turn_one_hand")
    nodes, _ = npr.build_tree(n_board_cards=4, bet_sizes=tree[0], raise_sizes=tree[1])
    h = [np.concatenate([h[0], [[TURN[3] + 1, 40]]]).astype(np.uint8), h[1]]       # a second hand of player 0 ...
    game = nbr.Game(TURN, h)
    game.blocked[0][:, 1] = True                                                   # ... that is dealt on no run-out
    game.W[:, 1, :] = 0.0
    cids = [[np.concatenate([c[0], c[0]], axis=1), c[1]] for c in cids]
    rng = np.random.Generator(np.random.PCG64(71))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = gadget_inputs(rng, 2)
    G = dict(resolver=1, alt=alt, regret=gr.copy(), ssum=gs.copy())
    R, S = copy_tables(*before)
    nr.gadget_sweep(nodes, R, S, G, game, cids, 0)
    assert (G["regret"][:, 1] == gr[:, 1]).all() and (G["ssum"][:, 1] == gs[:, 1]).all() and (G["ssum"][:, 0] != gs[:, 0]).any()
    for nd in nodes:
        if nd["kind"] == "action" and nd["player"] == 1:
            assert R[nd["index"]].tobytes() == before[0][nd["index"]].tobytes() and S[nd["index"]].tobytes() == before[1][nd["index"]].tobytes()
    kept = (G["regret"].copy(), G["ssum"].copy())
    nr.gadget_sweep(nodes, R, S, G, game, cids, 1)
    assert G["regret"].tobytes() == kept[0].tobytes() and G["ssum"].tobytes() == kept[1].tobytes()


# ---- d ---------------------------------------------------------------------------------------------------------------------------------------------------------
SAFETY = dict(trunk_iterations=5, node=2, prefix=0, resolver=0, iterations=50)


def safety_game():
    """the river game of test_200_iterations_solve_the_river_game (25 x 20 hands, one info set per hand) as a JOINT trunk with unit weights"""
    board0, h, cids, sizes, tree = make_case("river_lanes")
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])
    return board0, h, cids, sizes, tree, nodes, nw.WeightedGame(board0, h, (None, None), "joint")


def opponents_best_response(nodes, S, game, cids, resolver):
    sig = {i: nbr.final_strategy(s) for i, s in S.items()}
    return float(nbr.best_response(nodes, sig.__getitem__, None, None, cids, "max", None, game)[1 - resolver])


def unsafe_inputs(nodes, tables, game, cids, pre):
    """the recipe without the gadget: the opponent's weights are its own trunk reach (times its prior of ones), hands of weight 0 dropped"""
    P, O = pre["resolver"], 1 - pre["resolver"]
    node = int(pre["node_map"][0])
    own = nnr.report(nodes, nnr.strategies(tables).__getitem__, game, cids, O)[node]["own"][0]
    keep = own != 0.0
    hands, weights, clusters = list(pre["hands"]), list(pre["weights"]), [list(row) for row in pre["clusters"]]
    hands[O], weights[O] = game.hands[O][keep], own[keep]
    for r in range(len(clusters)):
        clusters[r][O] = np.asarray(cids[pre["round0"] + r][O]).reshape(-1, game.n[O])[:, keep]
    return dict(pre, hands=hands, weights=weights, clusters=clusters)


def test_grafting_a_gadget_resolve_does_not_raise_the_opponents_best_response():
    """Trunk: 5 iterations of plain CFR from zero tables (coarse on purpose).  Node 2 is player 1's node after player 0's check; the resolver, player 0, reaches it with
    all 25 hands.  The gadget game is trained 50 iterations from zero tables and player 0's rows are grafted (lane clusters: legal).  Player 1's best-response value
    against player 0 (np_br.best_response "max", chips per deal), measured with this restatement:
        safe (gadget):     54.545704 -> 46.203789       asserted: it does not rise, and here falls
        unsafe (no gadget, opponent weights own_O * prior_O):  54.545704 -> 43.590819       recorded, no order asserted"""
    board0, h, cids, sizes, tree, nodes, game = safety_game()
    R, S = nrc.zero_tables(nodes, sizes)
    nrc.train(nodes, R, S, game, cids, SAFETY["trunk_iterations"])
    P = SAFETY["resolver"]
    before = opponents_best_response(nodes, S, game, cids, P)
    pre = nr.prepare(nodes, (R, S), board0, h, cids, SAFETY["node"], SAFETY["prefix"], P, game=game)
    assert len(pre["hands"][P]) == 25 and len(pre["hands"][1 - P]) == 20
    results = {}
    for kind in ("safe", "unsafe"):
        pp = pre if kind == "safe" else unsafe_inputs(nodes, (R, S), game, cids, pre)
        sub_game = nw.WeightedGame(pp["board"], pp["hands"], pp["weights"], "joint")
        Rs, Ss = nrc.zero_tables(pp["nodes"], sizes)
        if kind == "safe":
            nr.gadget_train(pp["nodes"], Rs, Ss, nr.new_gadget(P, pp["alt"]), sub_game, pp["clusters"], SAFETY["iterations"])
        else:
            nrc.train(pp["nodes"], Rs, Ss, sub_game, pp["clusters"], SAFETY["iterations"])
        grafted = copy_tables(R, S)
        nr.graft((Rs, Ss), grafted, pp, P)
        results[kind] = opponents_best_response(nodes, grafted[1], game, cids, P)
    print("opponent's best response: trunk", before, "safe", results["safe"], "unsafe", results["unsafe"])
    assert abs(before - 54.545704) < 1e-5 and abs(results["safe"] - 46.203789) < 1e-5 and abs(results["unsafe"] - 43.590819) < 1e-5
    assert results["safe"] < before


# ---- e ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_two_summation_orders_of_a_gadget_sweep_stay_within_the_cell_rule(name):
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    cells, differ = order_check(name, nodes, cids, sizes, nbr.Game(board0, h))
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
