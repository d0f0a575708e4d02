"""The max-margin gadget and the per-hand root values of the best-response walk: their numpy restatement (tests/np_maxmargin.py) against its own second summation
order, the definitions' identities, and the behaviour that separates max-margin from CFR-D.  No device.

  1  two summation orders of a max-margin sweep stay within test_range_cfr_cpu.compare_cells' rule, the gadget's 2 n cells (row 0 of regret and ssum) counted with the
     table's, at most 0.5 % of a case's cells differing at all: what entitles tests/test_gpu_maxmargin.py to the same cap on the device
  2  units: under the trunk's own profile with alt = the profile's values every live margin is 0
  3  the resolver's sweep value is the rho-weighted margin under the current profile
  4  dead hands: cells untouched, rho 0, margin NaN; a range of one live hand has rho = 1
  5  behaviour on test_resolve_cpu.safety_game
"""
import numpy as np
import pytest

import np_maxmargin as nm
import np_node_report as nnr
import np_range_cfr as nrc
import np_resolve as nr
import np_weighted as nw
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_gpu_range_cfr import make_case
from test_np_br_cpu import ATOL, RIVER, RTOL, TURN, pick_ranges, random_cids
from test_range_cfr_cpu import RIVER_TREE, compare_cells, random_tables
from test_resolve_cpu import CASES, copy_tables, gadget_inputs, safety_game, turn_trunk

MM_CASES = CASES + ["river_hands_300"]


def mm_case(name):
    """test_gpu_range_cfr.make_case and river_hands_300: ranges beyond 256 hands, the second trip of a one-workgroup loop over the hands"""
    if name != "river_hands_300":
        return make_case(name)
    rng = np.random.Generator(np.random.PCG64(7))
    h = pick_ranges(rng, RIVER, 300, 290)
    return RIVER, h, random_cids(rng, RIVER, h, [(40, 37)]), [(40, 37)], RIVER_TREE


def mm_inputs(rng, n, rows="random"):
    """gadget_inputs' draw with its 1e30 entries replaced by a moderate value: they would drown every other term of U"""
    alt, regret, ssum = gadget_inputs(rng, n, rows)
    return np.where(alt > 1e29, 7.5, alt), regret, ssum


def tree_of(board0, tree):
    return npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])[0]


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------------------
def mm_order_check(name, nodes, cids, sizes, game, seed=351):
    """both resolvers, both traversers, plain and RM+, random and zero gadget rows -> (cells, cells that differ at all)"""
    cells = differ = 0
    for P in (0, 1):
        for p in (0, 1):
            for rmplus in (False, True):
                for rows in ("random", "zero"):
                    rng = np.random.Generator(np.random.PCG64(seed + 8 * P + 4 * p + 2 * rmplus + (rows == "zero")))
                    R, S = random_tables(rng, nodes, sizes)
                    alt, gr, gs = mm_inputs(rng, game.n[1 - P], rows)
                    out = []
                    for reverse in (False, True):
                        Rk, Sk = copy_tables(R, S)
                        G = dict(resolver=P, alt=alt, regret=gr.copy(), ssum=gs.copy(), margin=None)
                        v = nm.maxmargin_sweep(nodes, Rk, Sk, G, game, cids, p, rmplus, reverse=reverse)
                        out.append((v, Rk, Sk, G))
                    (v1, R1, S1, G1), (v2, R2, S2, G2) = out
                    assert abs(v1 - v2) <= RTOL * abs(v1) + ATOL, (name, P, p, rmplus, rows, v1, v2)
                    for G in (G1, G2):
                        assert G["regret"][1].tobytes() == gr[1].tobytes() and G["ssum"][1].tobytes() == gs[1].tobytes(), "row 1 is never written"
                    if p != P:
                        m1, m2 = G1["margin"], G2["margin"]
                        assert (np.isnan(m1) == np.isnan(m2)).all() and np.allclose(m1[~np.isnan(m1)], m2[~np.isnan(m2)], rtol=RTOL, atol=ATOL)
                    pairs = [(R1[i], R2[i]) for i in R1] + [(S1[i], S2[i]) for i in S1] + [(G1["regret"][0], G2["regret"][0]), (G1["ssum"][0], G2["ssum"][0])]
                    for a, b in pairs:
                        d, _ = compare_cells(a, b, (name, P, p, rmplus, rows))
                        cells += d.size
                        differ += int((d > 0).sum())
    return cells, differ


@pytest.mark.parametrize("name", MM_CASES)
def test_two_summation_orders_of_a_maxmargin_sweep_stay_within_the_cell_rule(name):
    board0, h, cids, sizes, tree = mm_case(name)
    cells, differ = mm_order_check(name, tree_of(board0, tree), cids, sizes, nbr.Game(board0, h))
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round0", [0, 1])
def test_under_the_trunks_own_profile_every_live_margin_is_zero(round0):
    """test_resolve_cpu's units check for this gadget: prepare(current=True) at turn-round and river-round nodes, the trunk's rows copied into the subgame, one sweep of
    the opponent from zero rows: |margin[h]| <= 1e-9 * max|alt| for every live hand (F / M and alt are the same sums in two f64 orders)"""
    nodes, h, cids, sizes, game, tables = turn_trunk()
    picked = [i for i, nd in enumerate(nodes) if nd["kind"] == "action" and nd["round_idx"] == round0]
    picked = [picked[0], picked[len(picked) // 2], picked[-1]]
    checked = 0
    for node in picked:
        for prefix in ([0] if round0 == 0 else [0, 5, 17, 47]):
            for P in (0, 1):
                pre = nr.prepare(nodes, tables, TURN, h, cids, node, prefix, P, current=True, game=game)
                sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
                R, S = nr.sub_tables(tables, pre)
                G = nm.new_gadget(P, pre["alt"])
                detail = {}
                U = nm.maxmargin_sweep(pre["nodes"], R, S, G, sub_game, pre["clusters"], 1 - P, detail=detail)
                live = detail["live"]
                bound = 1e-9 * np.abs(pre["alt"][live]).max()
                assert bound > 0 and (np.abs(G["margin"][live]) <= bound).all(), (node, prefix, P, np.abs(G["margin"][live]).max(), bound)
                assert np.isnan(G["margin"][~live]).all() and abs(U) <= bound
                checked += int(live.sum())
    assert checked > 30


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["river_lanes", "turn_imperfect_recall", "turn_no_opponent"])
def test_the_resolvers_sweep_value_is_the_rho_weighted_margin(name):
    """value = sum over live h of rho[h] * (alt[h] - F'[h] / M[h]), F' the fold of an opponent's walk of the same tables (the game is zero-sum)"""
    board0, h, cids, sizes, tree = mm_case(name)
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    for P in (0, 1):
        O = 1 - P
        rng = np.random.Generator(np.random.PCG64(361 + P))
        before = random_tables(rng, nodes, sizes)
        alt, gr, gs = mm_inputs(rng, game.n[O])
        G = dict(resolver=P, alt=alt, regret=gr.copy(), ssum=gs.copy(), margin=None)
        detail = {}
        value = nm.maxmargin_sweep(nodes, *copy_tables(*before), G, game, cids, P, detail=detail)
        vF = nr.walk(nodes, *copy_tables(*before), game, cids, O, np.ones((len(game.ro), game.n[P])))
        F = nm._fold(vF, ~game.blocked[O])
        rho, live, M = detail["rho"], detail["live"], detail["M"]
        want = float((rho[live] * (alt[live] - F[live] / M[live])).sum())
        print(name, P, value, want)
        assert abs(value - want) <= RTOL * abs(want) + ATOL, (name, P, value, want)
        assert live.any() and abs(rho.sum() - 1.0) < 1e-12


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_dead_hands_keep_their_cells_and_one_live_hand_has_rho_one():
    # (a) turn_no_opponent: hands 0 and 1 of player 0 meet no opponent on any lane: M = 0
    board0, h, cids, sizes, tree = mm_case("turn_no_opponent")
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    rng = np.random.Generator(np.random.PCG64(371))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = mm_inputs(rng, game.n[0])
    gr[0, :2] = 5.0                                                                # positive regrets on dead hands count for nothing
    for rmplus in (False, True):
        G = dict(resolver=1, alt=alt, regret=gr.copy(), ssum=gs.copy(), margin=None)
        detail = {}
        nm.maxmargin_sweep(nodes, *copy_tables(*before), G, game, cids, 0, rmplus, detail=detail)
        assert not detail["live"][:2].any() and detail["live"][2:].all() and (detail["M"][:2] == 0).all()
        assert (detail["rho"][:2] == 0).all() and abs(detail["rho"].sum() - 1.0) < 1e-12
        assert np.isnan(G["margin"][:2]).all() and np.isfinite(G["margin"][2:]).all()
        assert G["regret"][:, :2].tobytes() == gr[:, :2].tobytes() and G["ssum"][:, :2].tobytes() == gs[:, :2].tobytes()
        assert (G["ssum"][0, 2:] != gs[0, 2:]).any()
        d2 = {}
        nm.maxmargin_sweep(nodes, *copy_tables(*before), dict(G, regret=gr.copy(), ssum=gs.copy()), game, cids, 1, rmplus, detail=d2)
        assert (d2["rho"][:2] == 0).all()
    # (b) a hand blocked on every run-out, beside ONE live hand: rho = (1, 0) whatever the regrets
    board0, h, cids, sizes, tree = mm_case("turn_one_hand")
    nodes = tree_of(board0, tree)
    h = [np.concatenate([h[0], [[TURN[3] + 1, 40]]]).astype(np.uint8), h[1]]
    game = nbr.Game(TURN, h)
    game.blocked[0][:, 1] = True
    game.W[:, 1, :] = 0.0
    cids = [[np.concatenate([c[0], c[0]], axis=1), c[1]] for c in cids]
    before = random_tables(rng, nodes, sizes)
    for r0 in (-3.0, 0.0, 2.5):
        gr = np.array([[r0, 9.0], [1.0, 1.0]], dtype=np.float32)
        gs = np.array([[0.5, 0.25], [3.0, 4.0]], dtype=np.float32)
        G = dict(resolver=1, alt=np.array([4.0, -2.0]), regret=gr.copy(), ssum=gs.copy(), margin=None)
        detail = {}
        U = nm.maxmargin_sweep(nodes, *copy_tables(*before), G, game, cids, 0, detail=detail)
        assert detail["rho"].tolist() == [1.0, 0.0] and detail["live"].tolist() == [True, False]
        assert G["regret"][:, 1].tobytes() == gr[:, 1].tobytes() and G["ssum"][:, 1].tobytes() == gs[:, 1].tobytes() and np.isnan(G["margin"][1])
        assert G["ssum"][0, 0] == np.float32(1.5) and G["regret"][0, 0] == gr[0, 0]   # u - U = 0 with one live hand
        assert U == -G["margin"][0]


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------------------
def profile_margins(pre, Ss, alt):
    """the check of a re-solve: alt - value / mass per opponent hand, value / mass its best response in the real game against the average strategy of Ss"""
    sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
    sig = {i: nbr.final_strategy(s) for i, s in Ss.items()}
    value, mass = nm.root_hands(pre["nodes"], sig.__getitem__, sub_game, pre["clusters"], 1 - pre["resolver"], "max", real=True)
    return np.where(mass > 0, alt - value / np.where(mass > 0, mass, 1.0), np.nan)


def best_response_alt(pre, tables):
    sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
    _, S = nr.sub_tables(tables, pre)
    sig = {i: nbr.final_strategy(s) for i, s in S.items()}
    value, mass = nm.root_hands(pre["nodes"], sig.__getitem__, sub_game, pre["clusters"], 1 - pre["resolver"], "max", real=True)
    return np.where(mass > 0, value / np.where(mass > 0, mass, 1.0), 0.0)


MM_SAFETY = dict(node=2, prefix=0, resolver=0, trunk_iterations=50, iterations=200)
MEASURED = dict(cfrd=-4.897507, maxmargin=-3.746762)                              # see the docstring below


def safety_trunk(iterations):
    board0, h, cids, sizes, tree, nodes, game = safety_game()
    R, S = nrc.zero_tables(nodes, sizes)
    nrc.train(nodes, R, S, game, cids, iterations)
    pre = nr.prepare(nodes, (R, S), board0, h, cids, MM_SAFETY["node"], MM_SAFETY["prefix"], MM_SAFETY["resolver"], game=game)
    return nodes, sizes, (R, S), pre


def test_maxmargin_raises_the_smallest_margin_above_cfr_ds():
    """The safety game (river, 25 x 20 hands, one info set per hand, resolver 0, node 2), trunk: 50 plain iterations, alt = the profile's values, 200 plain iterations of the
    gadget game from zero tables.  The smallest per-hand best-response margin of player 1 against the re-solved average strategy, chips per unit mass, measured with
    this restatement:
        CFR-D (np_resolve.gadget_train)        -4.897507
        max-margin (np_maxmargin)              -3.746762
    asserted to 1e-5 each, and: max-margin's exceeds CFR-D's by at least half that gap.  (With the profile's values as alt the margins start negative: a best response
    beats the profile.  The next test uses the best-response alt.)"""
    nodes, sizes, trunk, pre = safety_trunk(MM_SAFETY["trunk_iterations"])
    P = pre["resolver"]
    sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
    got = {}
    for kind in ("cfrd", "maxmargin"):
        Rs, Ss = nrc.zero_tables(pre["nodes"], sizes)
        if kind == "cfrd":
            nr.gadget_train(pre["nodes"], Rs, Ss, nr.new_gadget(P, pre["alt"]), sub_game, pre["clusters"], MM_SAFETY["iterations"])
        else:
            nm.maxmargin_train(pre["nodes"], Rs, Ss, nm.new_gadget(P, pre["alt"]), sub_game, pre["clusters"], MM_SAFETY["iterations"])
        got[kind] = float(np.nanmin(profile_margins(pre, Ss, pre["alt"])))
    print("smallest margin: CFR-D %.6f max-margin %.6f" % (got["cfrd"], got["maxmargin"]))
    assert abs(got["cfrd"] - MEASURED["cfrd"]) < 1e-5 and abs(got["maxmargin"] - MEASURED["maxmargin"]) < 1e-5, got
    assert got["maxmargin"] - got["cfrd"] >= 0.5 * (MEASURED["maxmargin"] - MEASURED["cfrd"]) > 0


@pytest.mark.parametrize("trunk_iterations", [5, 50])
def test_maxmargin_with_best_response_alt_is_safe_for_every_hand(trunk_iterations):
    """alt = the opponent's counterfactual best-response values against the trunk (root_hands on the trunk's rows), 200 iterations with DCFR (1.5, 0, 2): the smallest
    margin is >= -1e-5; 0 is the optimum, some hand cannot be hurt.  Measured with this restatement: 0.000000 for both trunks (asserted to 1e-5)."""
    nodes, sizes, trunk, pre = safety_trunk(trunk_iterations)
    alt = best_response_alt(pre, trunk)
    sub_game = nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint")
    Rs, Ss = nrc.zero_tables(pre["nodes"], sizes)
    nm.maxmargin_train(pre["nodes"], Rs, Ss, nm.new_gadget(pre["resolver"], alt), sub_game, pre["clusters"], MM_SAFETY["iterations"], dcfr=(1.5, 0.0, 2.0))
    smallest = float(np.nanmin(profile_margins(pre, Ss, alt)))
    print("trunk", trunk_iterations, "smallest margin %.9f" % smallest)
    assert smallest >= -1e-5 and abs(smallest - 0.0) < 1e-5


# ---- root_hands against the restatements it is modelled on --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["river_lanes", "turn_imperfect_recall", "turn_no_opponent"])
def test_root_hands_sums_to_the_best_response_and_equals_the_node_report_at_the_root(name):
    import np_locks as nl
    board0, h, cids, sizes, tree = mm_case(name)
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    _, S = random_tables(np.random.Generator(np.random.PCG64(381)), nodes, sizes)
    sig = {i: nbr.final_strategy(s) for i, s in S.items()}
    for mode, real in (("max", False), ("max", True), ("avg", False)):
        want = nl.best_response(nodes, sig.__getitem__, game, cids, mode, real=real)
        for p in (0, 1):
            value, mass = nm.root_hands(nodes, sig.__getitem__, game, cids, p, mode, real)
            assert abs(value.sum() - want[p]) <= 1e-12 * np.abs(value).sum() + ATOL, (name, mode, real, p)
            assert ((mass > 0) | (value == 0)).all()
            if mode == "avg":
                first = next(i for i, nd in enumerate(nodes) if nd["kind"] == "action")   # the root, below the chance nodes that pass through
                rep = nnr.report(nodes, sig.__getitem__, game, cids, p)[first]
                assert np.allclose(value, rep["value"][0], rtol=RTOL, atol=ATOL) and np.allclose(mass, rep["mass"][0], rtol=RTOL, atol=ATOL)
