"""CPU: the numpy restatement of full-width CFR over hand ranges (tests/np_range_cfr.py) against what the algorithm is known to do.

  * it reaches the exploitabilities a prototype of the definition reached on six small games (river and turn, one info set per lane and coarse / imperfect-recall
    clusters; CFR, RM+ and Discounted CFR), within 1 %;
  * the final strategy's two values cancel (the game is zero-sum);
  * one sweep leaves the opponent's rows and every info set without a dealt lane untouched;
  * a second summation order (info-set lanes and leaf sums reversed) moves a cell by at most one f32 ulp: the tolerance the GPU tests hold the device to.
The GPU tests (tests/test_gpu_range_cfr.py) compare the device with this restatement sweep by sweep."""
import numpy as np
import pytest

import np_range_cfr as nrc
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_np_br_cpu import ATOL, RIVER, TURN, lane_cids, pick_ranges, random_cids, sizes_of

RIVER_TREE = (((0.5, 1.0),), ((3.0,),))                  # the default river tree: 14 action nodes
TURN_TREE = (((1.0,), (1.0,)), ((), ()))                 # one bet size per street: 16 action nodes

GAMES = {
    # name: (board0, hands of player 0 and 1, clusters, tree, rmplus, dcfr, {iteration: exploitability in chips per deal})
    "river_lanes_cfr": (RIVER, 25, 20, "lanes", RIVER_TREE, False, None, {0: 79.69, 10: 14.19, 50: 3.64, 100: 1.83, 200: 0.901}),
    "river_lanes_rmplus": (RIVER, 25, 20, "lanes", RIVER_TREE, True, None, {0: 79.69, 10: 14.37, 50: 3.21, 100: 1.58, 200: 0.814}),
    "river_lanes_dcfr": (RIVER, 25, 20, "lanes", RIVER_TREE, False, (1.5, 0.0, 2.0), {0: 79.69, 10: 5.38, 50: 0.384, 100: 0.142, 200: 0.0292}),
    "river_coarse_cfr": (RIVER, 25, 20, [(6, 9)], RIVER_TREE, False, None, {0: 61.06, 10: 11.00, 50: 2.34, 100: 1.21, 200: 0.597}),
    "turn_lanes_cfr": (TURN, 9, 7, "lanes", TURN_TREE, False, None, {0: 50.87, 10: 12.12, 50: 2.52, 100: 1.32}),
    "turn_imperfect_recall_cfr": (TURN, 9, 7, [(3, 4), (5, 6)], TURN_TREE, False, None, {0: 49.99, 10: 10.43, 50: 2.32, 100: 1.16}),
}


def make_game(board0, n0, n1, clusters, tree):
    """ranges from PCG64(7); random clusters from the same generator"""
    rng = np.random.Generator(np.random.PCG64(7))
    h = pick_ranges(rng, board0, n0, n1)
    cids = lane_cids(board0, h) if clusters == "lanes" else random_cids(rng, board0, h, clusters)
    sizes = sizes_of(cids) if clusters == "lanes" else list(clusters)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    return nodes, h, cids, sizes, nbr.Game(board0, h)


def random_tables(rng, nodes, sizes):
    """regrets normal x {0.01, 1, 30} per cluster, strategy sums uniform [0, 10) with 15 % zeros"""
    R, S = nrc.zero_tables(nodes, sizes)
    for i in R:
        A, C = R[i].shape
        R[i] = (rng.standard_normal((A, C)) * rng.choice([0.01, 1.0, 30.0], size=C)[None, :]).astype(np.float32)
        s = rng.random((A, C)) * 10.0
        s[rng.random((A, C)) < 0.15] = 0.0
        S[i] = s.astype(np.float32)
    return R, S


def ulps_apart(a, b):
    """distance in f32 steps between finite cells of equal sign (0.0 and -0.0 are the same cell value)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("name", sorted(GAMES))
def test_restatement_reaches_the_recorded_exploitabilities(name):
    board0, n0, n1, clusters, tree, rmplus, dcfr, want = GAMES[name]
    nodes, h, cids, sizes, game = make_game(board0, n0, n1, clusters, tree)
    assert sum(nd["kind"] == "action" for nd in nodes) == (14 if len(board0) == 5 else 16)
    R, S = nrc.zero_tables(nodes, sizes)
    got = {0: nrc.exploitability(nodes, S, game, cids)}

    def after(t):
        if t in want:
            got[t] = nrc.exploitability(nodes, S, game, cids)

    nrc.train(nodes, R, S, game, cids, max(want), rmplus=rmplus, dcfr=dcfr, after=after)
    for t, e in want.items():
        assert abs(got[t] - e) <= 0.01 * e, (name, t, got[t], e)
    v = nrc.profile_value(nodes, S, game, cids)
    assert abs(v[0] + v[1]) < ATOL, v


@pytest.mark.parametrize("name", ["river_coarse_cfr", "turn_imperfect_recall_cfr", "turn_lanes_cfr"])
@pytest.mark.parametrize("p", [0, 1])
def test_one_sweep_touches_only_the_traversers_dealt_info_sets(name, p):
    """the opponent's rows, and the cells of a cluster id no lane uses (one is appended to every round), are bit for bit what they were"""
    board0, n0, n1, clusters, tree, _, _, _ = GAMES[name]
    nodes, h, cids, sizes, game = make_game(board0, n0, n1, clusters, tree)
    sizes = [(a + 1, b + 1) for a, b in sizes]                  # the last cluster of every round holds no lane
    rng = np.random.Generator(np.random.PCG64(3 + p))
    R, S = random_tables(rng, nodes, sizes)
    R0, S0 = {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}
    nrc.sweep(nodes, R, S, game, cids, p, rmplus=False)
    changed = 0
    for nd in nodes:
        if nd["kind"] != "action":
            continue
        i = nd["index"]
        if nd["player"] != p:
            assert R[i].tobytes() == R0[i].tobytes() and S[i].tobytes() == S0[i].tobytes(), i
            continue
        used = np.zeros(R[i].shape[1], dtype=bool)
        used[np.unique(game.infoset_of(cids, nd["round_idx"], p)[~game.blocked[p]])] = True
        assert not used[-1]
        assert R[i][:, ~used].tobytes() == R0[i][:, ~used].tobytes() and S[i][:, ~used].tobytes() == S0[i][:, ~used].tobytes(), i
        changed += int((R[i][:, used] != R0[i][:, used]).sum())
    assert changed > 0


ORDER_CASES = {
    # name: (board0, hands, clusters, tree): the shapes of the GPU tests
    "river_lanes": (RIVER, 25, 20, "lanes", RIVER_TREE),
    "river_70x66_two_clusters": (RIVER, 70, 66, [(2, 2)], RIVER_TREE),
    "turn_lanes": (TURN, 9, 7, "lanes", TURN_TREE),
    "turn_imperfect_recall": (TURN, 9, 7, [(3, 4), (5, 6)], TURN_TREE),
}


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_a_second_summation_order_moves_a_cell_by_at_most_one_ulp(name):
    """both traversers, plain and RM+, from random tables: reversed info-set lanes and leaf sums against the restatement's own order"""
    nodes, h, cids, sizes, game = make_game(*ORDER_CASES[name])
    cells = differ = 0
    for p in (0, 1):
        for rmplus in (False, True):
            rng = np.random.Generator(np.random.PCG64(11 + 2 * p + rmplus))
            R, S = random_tables(rng, nodes, sizes)
            R2, S2 = {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}
            v1 = nrc.sweep(nodes, R, S, game, cids, p, rmplus)
            v2 = nrc.sweep(nodes, R2, S2, game, cids, p, rmplus, reverse=True)
            assert abs(v1 - v2) <= 1e-11 * abs(v1) + ATOL
            for i in R:
                for a, b in ((R[i], R2[i]), (S[i], S2[i])):
                    d = ulps_apart(a, b)
                    assert d.max() <= 1, (name, p, rmplus, i, d.max())
                    cells += d.size
                    differ += int((d > 0).sum())
    assert differ <= 0.005 * cells, (differ, cells)             # the share the GPU tests allow; the worst seen here is 8 of 74 240 (turn, one info set per lane)
