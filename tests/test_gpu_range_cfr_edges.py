"""GPU (-m gpu): the full-width CFR sweep (rs_range_cfr_*) against tests/np_range_cfr.py where tests/test_gpu_range_cfr.py leaves it free.

  * list lengths at the steps of the own-node kernels: 63 / 64 / 65 / 128 / 129 lanes, one lane and empty clusters in the wave form (steps of 64), 16 / 17 / 8 / 9 / 1 lanes
    and an empty cluster between used ones in the thread form (steps of 8);
  * one round in the wave form and the other in the thread form in one sweep (two own-node kinds at one depth of the level plan), both ways round;
  * three rounds from a flop: 2 352 ordered run-outs, own reach carried through two chance levels;
  * nodes of 7 and of 8 = RS_MAX_ACTIONS actions, in both forms (every tree of the other file has 2 and 3 only);
  * tables drawn from test_range_cfr_cpu.edge_tables: columns whose positive f32 sum overflows, -0.0, subnormals, -3.4e38, NaN and cells beyond 2^24; +inf regrets of
    the opponent (a NaN reach); train() with Discounted CFR from such tables.
Every comparison is teacher-forced and of the other file's form: one sweep from uploaded tables, cells of the restatement's class and within one ulp or ATOL where finite
(test_range_cfr_cpu.compare_cells), at most 0.5 % of a case's cells differ at all, untouched cells keep their bytes (NaN payloads too), the same call twice gives the same
bits, level plan and depth-first walk give the same bits.  tests/test_range_cfr_cpu.py holds the restatement to the same rule against its own second summation order on
every shape here.  NOTES.md ("Full-width CFR pinned at its edges") has the cells compared, the cells that differed and the wall time per case on an MI355X, and the
mutants of rs_br.hip these cases catch."""
import numpy as np
import pytest

import np_range_cfr as nrc
import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from test_gpu_br_pinned import depth_first
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, make_case, same_tables
from test_np_br_cpu import ATOL, RTOL
from test_range_cfr_cpu import EDGE_SHAPES, assert_poison_reached, edge_tables, make_shape, poison_nodes, random_tables

pytestmark = pytest.mark.gpu

RS_MAX_ACTIONS = L.MAX_ACTIONS                        # include/rustsolver_amd.h, as the wrapper declares it


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def wave_form(game, h, sizes, r, p):
    """rs_br.hip br_wave_per_info_set for traverser p's nodes of round r: lanes (run-outs x hands) >= 32 x the table's clusters"""
    return len(game.ro) * len(h[p]) >= 32 * sizes[r][p]


# per case: the form (wave?) of (round, player) the case is there for
FORMS = {
    "river_wave_runs": {(0, 0): True, (0, 1): False}, "river_wave_runs_swapped": {(0, 0): False, (0, 1): True},
    "river_thread_runs": {(0, 0): False, (0, 1): False},
    "turn_mixed_forms": {(0, 0): False, (0, 1): False, (1, 0): True, (1, 1): True},
    "turn_mixed_forms_swapped": {(0, 0): True, (0, 1): True, (1, 0): False, (1, 1): False},
    "flop_three_rounds": {(r, p): True for r in range(3) for p in (0, 1)},
    "river_eight_actions_thread": {(0, 0): False, (0, 1): False}, "river_eight_actions_wave": {(0, 0): True, (0, 1): True},
    "river_seven_actions_thread": {(0, 0): False, (0, 1): False},
    "river_unused_cluster": {(0, 0): False, (0, 1): False}, "turn_imperfect_recall": {(r, p): True for r in range(2) for p in (0, 1)},
    "turn_lanes": {(0, 0): True, (0, 1): True, (1, 0): False, (1, 1): False}, "turn_no_opponent": {(r, p): True for r in range(2) for p in (0, 1)},
}


def value_matches(got, want):
    return np.isnan(got) if np.isnan(want) else bool(np.isclose(got, want, rtol=RTOL, atol=ATOL))


def no_minus_zero_or_nan(nodes, p, R):
    """no regret cell of traverser p is NaN or -0.0"""
    for nd in nodes:
        if nd["kind"] == "action" and nd["player"] == p:
            x = R[nd["index"]]
            if np.isnan(x).any() or (x.view(np.uint32) == 0x80000000).any():
                return False
    return True


def sweep_case(name, shape, starts, both_plans, poison=False):
    """one sweep from each start in `starts` ("random", "edges"): both traversers, plain and RM+, rank-order and pair-loop leaves, the level plan and, with both_plans, the
    depth-first walk bit for bit beside it; the same call twice gives the same bits.  Prints and returns (cells, cells that differ at all, largest ulp distance)"""
    board0, h, cids, sizes, tree = shape
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    for (r, p), wave in FORMS[name].items():
        assert wave_form(game, h, sizes, r, p) == wave, (name, r, p)
    dev = Device(board0, h, cids, sizes, tree)
    walks = {}
    bad = poison_nodes(nodes) if poison else ()
    cells = differ = worst = 0
    for start in starts:
        for p in (0, 1):
            for rmplus in (False, True):
                rng = np.random.Generator(np.random.PCG64(100 + 2 * p + rmplus))
                before = random_tables(rng, nodes, sizes) if start == "random" else edge_tables(rng, nodes, sizes, bad)
                if poison and start == "random":
                    for i in bad:
                        before[0][i][0, 1] = np.inf
                want = copy_tables(*before)
                with np.errstate(over="ignore", invalid="ignore"):
                    value = nrc.sweep(nodes, want[0], want[1], game, cids, p, rmplus)
                for sorted_showdowns in (True, False):
                    what = (name, start, p, rmplus, sorted_showdowns)
                    dev.upload(*before)
                    got_value = dev.solver(rmplus, sorted_showdowns).iterate(p)
                    got = dev.download()
                    assert value_matches(got_value, value), (what, got_value, value)
                    c, d, w = compare_sweep(nodes, game, cids, p, before, got, want, what)
                    cells, differ, worst = cells + c, differ + d, max(worst, w)
                    if sorted_showdowns:             # determinism: the same call from the same tables
                        dev.upload(*before)
                        again = dev.solver(rmplus, True).iterate(p)
                        assert again == got_value or (np.isnan(again) and np.isnan(got_value)), what
                        assert same_tables(dev.download(), got), what
                    if both_plans:
                        with depth_first():
                            key = (rmplus, sorted_showdowns)
                            if key not in walks:
                                walks[key] = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns)
                            dev.upload(*before)
                            walked = walks[key].iterate(p)
                            assert walks[key].launches() == -1
                        assert walked == got_value or (np.isnan(walked) and np.isnan(got_value)), what
                        assert same_tables(dev.download(), got), (what, "depth first")
                if poison and start == "random" and p == 0:       # what tests/test_range_cfr_cpu.py asserts of the restatement, of the device's last download
                    assert_poison_reached(nodes, game, cids, got[0], got[1], got_value, rmplus, what)
    assert dev.solver().launches() > 0
    for wk in walks.values():
        wk.destroy()
    dev.close()
    print("SEEN", name, "+".join(starts) + ("+poison" if poison else ""), "cells", cells, "differ", differ, "largest ulp distance beyond ATOL", worst)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    return cells, differ, worst


BOTH_PLANS = {"turn_mixed_forms", "turn_mixed_forms_swapped", "flop_three_rounds", "river_eight_actions_thread", "river_eight_actions_wave"}


@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_one_sweep_on_the_edge_shapes_equals_the_restatement(name):
    """random and edge tables on test_range_cfr_cpu.EDGE_SHAPES; each case asserts the own-node form (wave or thread per info set) it is there for"""
    shape = make_shape(name)
    nodes, _ = npr.build_tree(n_board_cards=len(shape[0]), bet_sizes=shape[4][0], raise_sizes=shape[4][1])
    widths = set(len(nd["children"]) for nd in nodes if nd["kind"] == "action")
    if "eight" in name:
        assert RS_MAX_ACTIONS in widths and max(widths) == RS_MAX_ACTIONS
    if "seven" in name:
        assert max(widths) == 7
    if name.startswith("turn_mixed"):                # the two rounds take different kinds: two own-node launches at one depth of the level plan
        assert all(FORMS[name][0, p] != FORMS[name][1, p] for p in (0, 1))
    sweep_case(name, shape, ("random", "edges"), name in BOTH_PLANS)


@pytest.mark.parametrize("name", ["river_unused_cluster", "turn_imperfect_recall", "turn_lanes", "turn_no_opponent"])
def test_one_sweep_from_edge_tables_on_the_earlier_shapes(name):
    """tests/test_gpu_range_cfr.py's cases with unused clusters, imperfect recall, one info set per lane and lanes without an opponent, from edge_tables"""
    sweep_case(name, make_case(name), ("edges",), False)


@pytest.mark.parametrize("name", ["river_unused_cluster", "turn_imperfect_recall"])
def test_a_plus_inf_regret_of_the_opponent_reaches_what_it_should(name):
    """+inf in the regret of action 0 of cluster 1 of player 1's first-round nodes, over random and over edge tables: cell classes as the restatement's.  From the random
    tables, traverser 0: the value is NaN, every touched regret of the nodes the NaN reach arrives at is NaN (+0.0 under RM+), its other regrets and every strategy sum are
    finite (test_range_cfr_cpu.assert_poison_reached).  With nobody in cluster 1 the same cells reach nothing: everything else stays finite"""
    board0, h, cids, sizes, tree = make_case(name)
    sweep_case(name, (board0, h, cids, sizes, tree), ("random", "edges"), name.startswith("turn"), poison=True)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    bad = poison_nodes(nodes)
    cids = [[c.copy() for c in row] for row in cids]
    cids[0][1][cids[0][1] == 1] = 0                   # nobody is in cluster 1 any more
    dev = Device(board0, h, cids, sizes, tree)
    for p in (0, 1):
        for rmplus in (False, True):
            before = random_tables(np.random.Generator(np.random.PCG64(61 + p)), nodes, sizes)
            for i in bad:
                before[0][i][0, 1] = np.inf
            dev.upload(*before)
            assert np.isfinite(dev.solver(rmplus).iterate(p)), (name, p, rmplus)
            R, S = dev.download()
            for i in R:
                keep = np.ones(R[i].shape, dtype=bool)
                keep[0, 1] = i not in bad
                assert np.isfinite(R[i][keep]).all() and np.isfinite(S[i]).all(), (name, p, rmplus, i)
            assert all(np.isposinf(R[i][0, 1]) for i in bad)
    dev.close()


@pytest.mark.parametrize("name", ["river_thread_runs", "turn_imperfect_recall"])
def test_rmplus_leaves_plus_zero(name):
    """RS_UPD_RMPLUS from edge tables whose untouched cells hold no NaN and no -0.0 (the traverser's own rows are made positive where the sweep does not write): after the
    sweep no regret cell of the traverser is NaN or -0.0 -- `not > 0` becomes +0.0f, NaN included -- and the restatement agrees"""
    board0, h, cids, sizes, tree = make_shape(name) if name in EDGE_SHAPES else make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    dev = Device(board0, h, cids, sizes, tree)
    for p in (0, 1):
        before = edge_tables(np.random.Generator(np.random.PCG64(71 + p)), nodes, sizes)
        written = 0
        for nd in nodes:
            if nd["kind"] == "action" and nd["player"] == p:
                used = np.zeros(before[0][nd["index"]].shape[1], dtype=bool)
                used[np.unique(game.infoset_of(cids, nd["round_idx"], p)[~game.blocked[p]])] = True
                before[0][nd["index"]][:, ~used] = 1.0
                x = before[0][nd["index"]][:, used]
                written += int((np.isnan(x) | (x.view(np.uint32) == 0x80000000)).sum())
        assert written > 0 and not no_minus_zero_or_nan(nodes, p, before[0])          # the sweep has NaN and -0.0 cells to rewrite
        want = copy_tables(*before)
        with np.errstate(over="ignore", invalid="ignore"):
            nrc.sweep(nodes, want[0], want[1], game, cids, p, True)
        assert no_minus_zero_or_nan(nodes, p, want[0])
        for sorted_showdowns in (True, False):
            dev.upload(*before)
            dev.solver(True, sorted_showdowns).iterate(p)
            assert no_minus_zero_or_nan(nodes, p, dev.download()[0]), (name, p, sorted_showdowns)
    dev.close()


def test_train_with_dcfr_from_edge_tables_equals_sweeps_and_ticks_issued_one_by_one():
    """2 iterations with DCFR (1.5, 0, 2) from edge tables, poisoned as well: non-finite cells (NaN regrets, then NaN reach and values) do not part the two paths.
    (The poison lasts one iteration: player 1's own sweep turns the column's regrets into NaN -- or +0.0 under RM+ -- which are not played.)"""
    board0, h, cids, sizes, tree = make_shape("river_thread_runs")
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    for poison in (False, True):
        before = edge_tables(np.random.Generator(np.random.PCG64(81)), nodes, sizes, poison_nodes(nodes) if poison else ())
        for rmplus in (False, True):
            s = dev.solver(rmplus)
            dev.upload(*before)
            values = s.train(2, dcfr=True)
            whole = dev.download()
            dev.upload(*before)
            for t in (1, 2):
                one = [s.iterate(0), s.iterate(1)]
                if t == 1:
                    assert np.isnan(one).all() if poison else np.isfinite(one).all(), (poison, rmplus, one)
                dev.table.discount_dcfr(*rs.dcfr_factors(1.5, 0.0, 2.0, t))
            assert same_tables(dev.download(), whole), (poison, rmplus)
            assert np.array_equal(np.array(one), values, equal_nan=True), (poison, rmplus, one, values)
            assert np.isfinite(values).all(), (poison, rmplus, values)
            dev.upload(*before)
            s.train(2)
            assert not same_tables(dev.download(), whole)            # the ticks did something
    dev.close()
