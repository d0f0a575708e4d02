"""CPU: the numpy restatement of full-width CFR over hand ranges (tests/np_range_cfr.py) against what the algorithm is known to do.

  * it reaches the exploitabilities a prototype of the definition reached on six small games (river and turn, one info set per lane and coarse / imperfect-recall
    clusters; CFR, RM+ and Discounted CFR), within 1 %;
  * the final strategy's two values cancel (the game is zero-sum);
  * one sweep leaves the opponent's rows and every info set without a dealt lane untouched;
  * a second summation order (info-set lanes and leaf sums reversed) moves a cell by at most one f32 ulp: the tolerance the GPU tests hold the device to;
  * the same on the shapes and the edge tables of tests/test_gpu_range_cfr_edges.py (EDGE_SHAPES, edge_tables), cell classes (finite, +inf, -inf, NaN) equal;
  * what the numeric edges mean: an overflowing positive sum plays nothing, a NaN regret is not played, a +inf regret of the opponent makes its reach NaN.
The GPU tests (tests/test_gpu_range_cfr.py, tests/test_gpu_range_cfr_edges.py) compare the device with this restatement sweep by sweep.  NOTES.md ("Full-width CFR pinned
at its edges") has the figures seen."""
import numpy as np
import pytest

import np_range_cfr as nrc
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_np_br_cpu import ATOL, FLOP, RIVER, TURN, lane_cids, pick_ranges, random_cids, sizes_of

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


# the cell values of edge_tables: test_gpu_br_pinned.edge_sums' f32 pool with the signs a regret can have
REGRET_POOL = np.array([3.4e38, 3.0e38, 1.7e38, -3.4e38, 2.0**24 + 2, 977.25, 30.0, 1.0, 0.5, 0.0, -0.0, 1e-45, 3e-45, -1e-45, 1.1754942e-38, -5.0, -30.0, np.nan], dtype=np.float32)
SUM_POOL = np.array([3.4e38, 3.0e38, 1.7e38, 2.0**24 + 2, 977.25, 30.0, 1.0, 0.5, 0.0, -0.0, 1e-45, 3e-45, 1.1754942e-38], dtype=np.float32)   # its finite cells that are not < 0


def edge_tables(rng, nodes, sizes, poison=()):
    """every cell drawn from REGRET_POOL / SUM_POOL: columns whose positive f32 sum overflows (they play nothing), -0.0, subnormals, -3.4e38 and NaN (not positive: not
    played), cells beyond 2^24.  poison: indices of action nodes that get +inf in the regret of action 0 of cluster 1 (inf / inf: a NaN strategy), as edge_sums does"""
    R, S = nrc.zero_tables(nodes, sizes)
    for i in R:
        R[i] = REGRET_POOL[rng.integers(0, len(REGRET_POOL), R[i].shape)]
        S[i] = SUM_POOL[rng.integers(0, len(SUM_POOL), S[i].shape)]
        if i in poison and R[i].shape[1] > 1:
            R[i][0, 1] = np.inf
    return R, S


def cell_classes(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def compare_cells(got, want, what=None):
    """the class-aware cell rule of every range-CFR comparison: the classes (finite, +inf, -inf, NaN) are equal, and a finite cell is within one f32 ulp of the other or
    within ATOL absolutely.  Returns the ulp distances, 0 where the cells are not finite, and the same with 0 where the cells are within ATOL as well (two cells near 0.0
    are many steps apart)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    cg, cw = cell_classes(got), cell_classes(want)
    assert (cg == cw).all(), (what, "cell classes differ", np.argwhere(cg != cw)[:4].tolist(), got[cg != cw][:4], want[cg != cw][:4])
    fin = cw == 0
    d = np.where(fin, ulps_apart(np.where(fin, got, 0), np.where(fin, want, 0)), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.abs(np.where(fin, got, 0).astype(np.float64) - np.where(fin, want, 0).astype(np.float64)) <= ATOL
    assert ((d <= 1) | near).all(), (what, int(d.max()))
    return d, np.where(near, 0, d)


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


def order_check(name, nodes, cids, sizes, game, tables, seed, strict=False):
    """both traversers, plain and RM+: reversed info-set lanes and leaf sums against the restatement's own order, cell by cell under compare_cells; -> (cells, cells that differ).
    strict: the two values are finite and every cell is within ONE ulp, with no way out through ATOL (well-behaved tables)"""
    cells = differ = worst = 0
    for p in (0, 1):
        for rmplus in (False, True):
            rng = np.random.Generator(np.random.PCG64(seed + 2 * p + rmplus))
            R, S = tables(rng, nodes, sizes)
            R2, S2 = {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}
            with np.errstate(invalid="ignore", over="ignore"):
                v1 = nrc.sweep(nodes, R, S, game, cids, p, rmplus)
                v2 = nrc.sweep(nodes, R2, S2, game, cids, p, rmplus, reverse=True)
            if strict:
                assert abs(v1 - v2) <= 1e-11 * abs(v1) + ATOL, (name, p, rmplus, v1, v2)
            assert np.isnan(v1) == np.isnan(v2) and (np.isnan(v1) or abs(v1 - v2) <= 1e-11 * abs(v1) + ATOL), (name, p, rmplus, v1, v2)
            for i in R:
                for a, b in ((R[i], R2[i]), (S[i], S2[i])):
                    d, far = compare_cells(a, b, (name, p, rmplus, i))
                    if strict:
                        assert np.isfinite(a).all() and np.isfinite(b).all() and d.max() <= 1, (name, p, rmplus, i, d.max())
                    cells += d.size
                    differ += int((d > 0).sum())
                    worst = max(worst, int(far.max()))
    print(name, tables.__name__, "cells", cells, "differ", differ, "largest ulp distance beyond ATOL", worst)
    return cells, differ


@pytest.mark.parametrize("name", sorted(ORDER_CASES))
def test_a_second_summation_order_moves_a_cell_by_at_most_one_ulp(name):
    """both traversers, plain and RM+, from random tables: reversed info-set lanes and leaf sums against the restatement's own order"""
    nodes, h, cids, sizes, game = make_game(*ORDER_CASES[name])
    cells, differ = order_check(name, nodes, cids, sizes, game, random_tables, 11, strict=True)
    assert differ <= 0.005 * cells, (differ, cells)             # the share the GPU tests allow; seen here: no cell differs in any of the four cases


# ---- the shapes of tests/test_gpu_range_cfr_edges.py: list lengths at the steps of the own-node kernels, both forms in one sweep, three rounds, nodes of 7 and 8 actions ----
WIDE_TREE_8 = (((0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.65),), ((2.0,),))       # 44 action nodes of 2, 3 and 8 actions
WIDE_TREE_7 = (((0.1, 0.2, 0.3, 0.4, 0.5, 0.6),), ((2.0, 3.0),))         # 86 action nodes of 2, 4 and 7 actions
FLOP_TREE = (((0.5,),) * 3, ((),) * 3)
WAVE_RUNS, THREAD_RUNS = [64, 65, 1, 128, 129, 63], [16, 17, 0, 8, 1, 9]


def cut_cids(runs):
    """one round, one prefix: the hands of each player cut into info sets of the given run lengths (a run of 0: an info set without a lane between used ones)"""
    return [[np.repeat(np.arange(len(r), dtype=np.uint32), r)[None, :] for r in runs]]


def padded_lane_cids(n_prefixes, n_hands):
    """one info set per (prefix, hand)"""
    return [(np.arange(n_prefixes, dtype=np.uint32)[:, None] * n + np.arange(n, dtype=np.uint32)[None, :]) for n in n_hands]


def make_shape(name):
    """-> board0, hands, cids, table sizes, (bet sizes, raise sizes); ranges and clusters from PCG64(7)"""
    rng = np.random.Generator(np.random.PCG64(7))
    if name in ("river_wave_runs", "river_wave_runs_swapped"):       # 450 hands in runs at, below and above one and two wave steps, a single lane, two empty clusters after
        h = pick_ranges(rng, RIVER, sum(WAVE_RUNS), 40)
        cids, sizes = cut_cids((WAVE_RUNS, [8] * 5)), [(8, 5)]
        if name.endswith("swapped"):
            h, cids, sizes = h[::-1], [cids[0][::-1]], [(5, 8)]
        return RIVER, h, cids, sizes, RIVER_TREE
    if name == "river_thread_runs":                                  # steps of 8: two full steps, two and a lane, an EMPTY cluster between used ones, one step, one lane, 9
        h = pick_ranges(rng, RIVER, sum(THREAD_RUNS), sum(THREAD_RUNS))
        return RIVER, h, cut_cids((THREAD_RUNS, THREAD_RUNS)), [(6, 6)], RIVER_TREE
    if name == "turn_mixed_forms":                                   # first round: one info set per hand in a table too wide for the wave form; last round coarse
        h = pick_ranges(rng, TURN, 9, 7)
        last = random_cids(rng, TURN, h, [(1, 1), (5, 6)])[1]
        return TURN, h, [padded_lane_cids(1, (9, 7)), last], [(14, 11), (5, 6)], TURN_TREE
    if name == "turn_mixed_forms_swapped":                           # first round coarse, last round one info set per lane
        h = pick_ranges(rng, TURN, 9, 7)
        first = random_cids(rng, TURN, h, [(3, 4), (1, 1)])[0]
        return TURN, h, [first, padded_lane_cids(48, (9, 7))], [(3, 4), (48 * 9, 48 * 7)], TURN_TREE
    if name == "flop_three_rounds":                                  # 2 352 ordered run-outs, prefixes 1 / 49 / 2 352, imperfect recall
        h = pick_ranges(rng, FLOP, 12, 15)
        sizes = [(4, 3), (6, 5), (9, 7)]
        return FLOP, h, random_cids(rng, FLOP, h, sizes), sizes, FLOP_TREE
    if name in ("river_eight_actions_thread", "river_seven_actions_thread"):
        h = pick_ranges(rng, RIVER, 25, 20)
        cids = lane_cids(RIVER, h)
        return RIVER, h, cids, sizes_of(cids), WIDE_TREE_8 if "eight" in name else WIDE_TREE_7
    if name == "river_eight_actions_wave":
        h = pick_ranges(rng, RIVER, 70, 66)
        return RIVER, h, random_cids(rng, RIVER, h, [(2, 2)]), [(2, 2)], WIDE_TREE_8
    raise KeyError(name)


EDGE_SHAPES = ["river_wave_runs", "river_wave_runs_swapped", "river_thread_runs", "turn_mixed_forms", "turn_mixed_forms_swapped", "flop_three_rounds",
               "river_eight_actions_thread", "river_eight_actions_wave", "river_seven_actions_thread"]


def shape_game(name):
    board0, h, cids, sizes, tree = make_shape(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    return nodes, h, cids, sizes, nbr.Game(board0, h)


def test_the_edge_shapes_are_what_they_are_there_for():
    widths = lambda tree: sorted(set(len(nd["children"]) for nd in npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])[0] if nd["kind"] == "action"))
    assert widths(WIDE_TREE_8) == [2, 3, 8] and widths(WIDE_TREE_7) == [2, 4, 7]            # 8 is RS_MAX_ACTIONS
    assert sum(nd["kind"] == "action" for nd in npr.build_tree(n_board_cards=5, bet_sizes=WIDE_TREE_8[0], raise_sizes=WIDE_TREE_8[1])[0]) == 44
    _, h, cids, sizes, game = shape_game("river_wave_runs")
    assert np.bincount(cids[0][0][0], minlength=8).tolist() == WAVE_RUNS + [0, 0] and len(h[0]) == 450 and np.bincount(cids[0][1][0]).tolist() == [8] * 5
    _, h, cids, sizes, game = shape_game("river_thread_runs")
    assert np.bincount(cids[0][0][0]).tolist() == THREAD_RUNS == np.bincount(cids[0][1][0]).tolist()
    _, h, cids, sizes, game = shape_game("flop_three_rounds")
    assert [c[0].shape[0] for c in cids] == [1, 49, 2352] and len(game.ro) == 2352


@pytest.mark.parametrize("tables", ["random", "edges"])
@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_a_second_summation_order_on_the_edge_shapes(name, tables):
    """the reference alone stays inside what the GPU tests allow: classes equal, finite cells within one ulp or ATOL, at most 0.5 % of the cells differ at all
    (seen: one cell of 73 952 differs, by one ulp, in turn_mixed_forms_swapped from random tables; none in the other 17 runs: NOTES.md)"""
    nodes, h, cids, sizes, game = shape_game(name)
    cells, differ = order_check(name, nodes, cids, sizes, game, random_tables if tables == "random" else edge_tables, 11)
    assert cells > 0 and differ <= 0.005 * cells, (name, tables, differ, cells)


# ---- what the numeric edges mean in the restatement ----------------------------------------------------------------------------------------------------

def first_node_of(nodes, p):
    """the first action node of player p on the path of first actions from the root"""
    i = 0
    while nodes[i]["kind"] != "action" or nodes[i]["player"] != p:
        i = nodes[i]["children"][0]
    return nodes[i]


def copy_of(R, S):
    return {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}


def test_an_overflowing_positive_sum_plays_nothing():
    """river, one info set per hand; every column of player 0's root is (3.4e38, 3.0e38, 1): the positive sum is +inf, sigma a column of zeros.  The sweep is worth 0; the
    children's own reach is 0, so no strategy sum of player 0 moves; U is 0, so the regret moves by the action's sum S[a] alone -- which a second sweep with the column
    playing action 2 alone hands back as its value (one lane per info set: the same f64)"""
    nodes, h, cids, sizes, game = make_game(RIVER, 25, 20, "lanes", RIVER_TREE)
    root = first_node_of(nodes, 0)
    i0 = root["index"]
    assert len(root["children"]) == 3 and nodes[nodes[0]["children"][0]] is root
    R, S = random_tables(np.random.Generator(np.random.PCG64(51)), nodes, sizes)
    R[i0][:] = np.array([3.4e38, 3.0e38, 1.0], dtype=np.float32)[:, None]
    before = copy_of(R, S)
    with np.errstate(over="ignore"):
        assert (npr.get_strategy_f32(R[i0]) == 0).all()
        assert nrc.sweep(nodes, R, S, game, cids, 0) == 0.0
    moved = 0
    for nd in nodes:
        if nd["kind"] == "action" and nd["player"] == 0:
            assert S[nd["index"]].tobytes() == before[1][nd["index"]].tobytes(), nd["index"]
            moved += int((R[nd["index"]] != before[0][nd["index"]]).sum())
    assert moved > 0 and R[i0][:2].tobytes() == before[0][i0][:2].tobytes()           # (3.4e38 takes no sum of a few hundred chips)
    for c in (0, 7, 24):
        R2, S2 = copy_of(*before)
        R2[i0][:, c] = [0.0, 0.0, 1.0]
        with np.errstate(over="ignore"):
            s2 = nrc.sweep(nodes, R2, S2, game, cids, 0)
        assert s2 != 0.0 and R[i0][2, c] == np.float32(1.0 + s2), (c, s2, R[i0][2, c])


@pytest.mark.parametrize("rmplus", [False, True])
def test_a_nan_regret_is_not_played(rmplus):
    """NaN > 0 is false: the cell is not summed and not played; it stays NaN without RM+ (NaN + x) and becomes +0.0 with it (NaN is not > 0)"""
    nodes, h, cids, sizes, game = make_game(RIVER, 25, 20, [(6, 9)], RIVER_TREE)
    root = first_node_of(nodes, 0)
    i0 = root["index"]
    R, S = random_tables(np.random.Generator(np.random.PCG64(52)), nodes, sizes)
    R[i0][:, 2] = [np.nan, 2.0, 6.0]
    assert npr.get_strategy_f32(R[i0])[:, 2].tolist() == [0.0, 0.25, 0.75]
    S0 = S[i0].copy()
    with np.errstate(invalid="ignore"):
        v = nrc.sweep(nodes, R, S, game, cids, 0, rmplus)
    assert np.isfinite(v) and np.isfinite(R[i0][1:, 2]).all() and np.isfinite(S[i0]).all()
    assert S[i0][0, 2] == S0[0, 2] and S[i0][1, 2] > S0[1, 2]                                 # the reach of the column went to actions 1 and 2
    if rmplus:
        assert R[i0][0, 2].tobytes() == np.float32(0.0).tobytes()
    else:
        assert np.isnan(R[i0][0, 2])
    R[i0][0, 2] = 0.0
    assert all(np.isfinite(x).all() for x in R.values())


def poison_nodes(nodes):
    """player 1's nodes of the first round"""
    return [nd["index"] for nd in nodes if nd["kind"] == "action" and nd["player"] == 1 and nd["round_idx"] == 0]


def nodes_the_poison_reaches(nodes, poison):
    """player 0's nodes whose sums meet the NaN reach: those above a poisoned node (U takes the NaN of that action into every regret of the info set) and those below a
    poisoned node's action 0.  Its other actions are played with 0 (finite / inf): below them the cluster's lanes carry nothing, until the next poisoned node (0 * NaN)"""
    out = set()

    def walk(i, under):
        nd = nodes[i]
        if nd["kind"] == "terminal":
            return False
        here = nd["kind"] == "action" and nd["player"] == 1 and nd["index"] in poison
        has = [walk(ch, under or (here and a == 0)) for a, ch in enumerate(nd["children"])]
        if nd["kind"] == "action" and nd["player"] == 0 and (under or any(has)):
            out.add(nd["index"])
        return here or any(has)

    walk(0, False)
    return out


def assert_poison_reached(nodes, game, cids, R, S, value, rmplus, what):
    """after traverser 0's sweep from finite tables against +inf regrets in player 1's first round: the value is NaN; at the nodes the poison reaches every regret cell of
    an info set with a dealt lane is NaN, or +0.0 under RM+, at player 0's other nodes finite; the strategy sums are finite (the traverser's own reach never reads the
    opponent's strategy)"""
    assert np.isnan(value), (what, value)
    reached = nodes_the_poison_reaches(nodes, poison_nodes(nodes))
    assert reached
    for nd in nodes:
        if nd["kind"] != "action" or nd["player"] != 0:
            continue
        i = nd["index"]
        used = np.zeros(R[i].shape[1], dtype=bool)
        used[np.unique(game.infoset_of(cids, nd["round_idx"], 0)[~game.blocked[0]])] = True
        assert used.any()
        if i not in reached:
            assert np.isfinite(R[i]).all(), (what, i)
        elif rmplus:
            assert (R[i][:, used].view(np.uint32) == 0).all(), (what, i)
        else:
            assert np.isnan(R[i][:, used]).all(), (what, i)
        assert np.isfinite(S[i]).all(), (what, i)


POISON_SHAPES = {"river": (RIVER, 25, 20, [(6, 9)], RIVER_TREE), "turn": (TURN, 9, 7, [(3, 4), (5, 6)], TURN_TREE)}


@pytest.mark.parametrize("rmplus", [False, True])
@pytest.mark.parametrize("shape", sorted(POISON_SHAPES))
def test_a_plus_inf_regret_of_the_opponent_makes_its_reach_nan(shape, rmplus):
    """+inf in action 0 of cluster 1 of every first-round node of player 1: inf / inf.  Every info set of player 0 meets a lane of that cluster below its root (asserted by
    what follows), so the sweep's value and every touched regret of the nodes the NaN reach arrives at are NaN (+0.0 under RM+) while the strategy sums stay finite.  In a cluster no lane uses it reaches nothing"""
    nodes, h, cids, sizes, game = make_game(*POISON_SHAPES[shape])
    assert nodes[first_node_of(nodes, 0)["children"][0]]["index"] in poison_nodes(nodes)
    R, S = random_tables(np.random.Generator(np.random.PCG64(53)), nodes, sizes)
    for i in poison_nodes(nodes):
        R[i][0, 1] = np.inf
    before = copy_of(R, S)
    with np.errstate(invalid="ignore"):
        v = nrc.sweep(nodes, R, S, game, cids, 0, rmplus)
    assert_poison_reached(nodes, game, cids, R, S, v, rmplus, shape)
    cids[0][1][cids[0][1] == 1] = 0                                   # nobody is in cluster 1 any more
    R, S = before
    with np.errstate(invalid="ignore"):
        v = nrc.sweep(nodes, R, S, game, cids, 0, rmplus)
    assert np.isfinite(v) and all(np.isfinite(S[i]).all() for i in S)
    assert all(np.isfinite(R[i]).all() for i in R if i not in poison_nodes(nodes))


def adopt_tree(nodes):
    """np_restate.build_tree's nodes as the library's records (rs_tree_from_nodes): the way to a node of RS_MAX_ACTIONS actions, which takes more bet sizes than
    rs_options holds (RS_MAX_SIZES).  Host only; the GPU files import it from here"""
    import rustsolver_amd as rs
    from rustsolver_amd import _lib as L
    kinds = {"private_chance": L.NODE_PRIVATE_CHANCE, "public_chance": L.NODE_PUBLIC_CHANCE, "action": L.NODE_ACTION, "terminal": L.NODE_TERMINAL}
    acts = {"bet": L.ACT_BET, "raise": L.ACT_RAISE, "check": L.ACT_CHECK, "call": L.ACT_CALL, "fold": L.ACT_FOLD}
    terms = {"ALLIN": L.TERM_ALLIN, "SHOWDOWN": L.TERM_SHOWDOWN, "UNCONTESTED": L.TERM_UNCONTESTED}
    out = []
    for nd in nodes:
        t = L.TreeNode()
        t.kind, t.parent, t.n_children, t.index = kinds[nd["kind"]], nd["parent"], len(nd["children"]), -1
        for k, c in enumerate(nd["children"]):
            t.children[k] = c
        if nd["kind"] == "action":
            t.index, t.player, t.round_idx = nd["index"], nd["player"], nd["round_idx"]
            for k, (kind, amt) in enumerate(nd["actions"]):
                t.action_kind[k], t.action_amt[k] = acts[kind], amt
        elif nd["kind"] == "terminal":
            t.value, t.ttype, t.last_to_act, t.round = nd["value"], terms[nd["ttype"]], nd["last_to_act"], nd["round"]
        elif nd["kind"] == "public_chance":
            t.round = nd["round"]
        out.append(t)
    return rs.tree_from_nodes(out)


def test_adopted_trees_are_the_built_ones():
    """adopt_tree (the restated nodes through rs_tree_from_nodes -- the way to the 7- and 8-action trees, whose bet sizes rs_options cannot hold) gives
    rs_tree_build's records byte for byte where both can build the tree; the widest node is RS_MAX_ACTIONS wide; no GPU needed"""
    import rustsolver_amd as rs
    from rustsolver_amd import _lib as L
    assert L.MAX_ACTIONS == 8
    for n_board, (bets, raises) in ((5, RIVER_TREE), (4, TURN_TREE), (3, FLOP_TREE), (4, (((0.25, 0.5, 1.0, 2.0),) * 2, ((2.0, 3.0),) * 2))):
        _, built = rs.build_game_tree(rs.Options(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises))
        adopted = adopt_tree(npr.build_tree(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises)[0])
        assert adopted.n_nodes == built.n_nodes and all(bytes(a) == bytes(b) for a, b in zip(adopted.nodes, built.nodes)), n_board
    for tree, n_action, widest in ((WIDE_TREE_8, 44, 8), (WIDE_TREE_7, 86, 7)):
        adopted = adopt_tree(npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])[0])
        assert adopted.n_action_nodes == n_action and max(nd.n_children for nd in adopted.action_nodes()) == widest
