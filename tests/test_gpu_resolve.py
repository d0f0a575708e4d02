"""GPU (-m gpu): safe subgame re-solving -- rs_tree_subtree, the re-solving gadget of the full-width solver (rs_range_cfr_set_gadget / _gadget_get / _gadget_set) and
rustsolver_amd.resolve -- against the numpy restatement tests/np_resolve.py.

Teacher-forced like tests/test_gpu_range_cfr.py: the restatement's tables and gadget rows are uploaded, the device does ONE sweep, and the result is compared with the
restatement's own next state.  Per cell the rule is test_range_cfr_cpu.compare_cells (class, one f32 ulp, or ATOL), the gadget's 4 n cells counted with the table's; at
most 0.5 % of a case's cells may differ at all; tests/test_resolve_cpu.py holds the restatement's two summation orders to the same rule on the same cases (run here
first, per case).  Cells a sweep must not touch are bit-equal to the upload: the resolver's rows on the opponent's sweep, the gadget rows on the resolver's, the cells
of hands without a dealt lane always.

Shapes, each the smallest that reaches a branch of the gadget kernels: river_lanes (NB = 1, 20 / 25 hands: under one wave), river_wave_35 (66 / 70 hands: a ragged
second wave), turn_lanes and turn_imperfect_recall (NB = 48: the fold, lanes blocked by the turn card, flight steps of 8 dividing 48 -- and 47 dealt run-outs not),
turn_one_hand (a range of one hand, as resolver and as opponent), turn_no_opponent (opponent hands whose mass is 0 on every lane)."""
import numpy as np
import pytest

import np_range_cfr as nrc
import np_resolve as nr
import np_weighted as nw
import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from rustsolver_amd import resolve
from test_gpu_br_pinned import depth_first
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, make_case, same_tables
from test_np_br_cpu import ATOL, RTOL
from test_range_cfr_cpu import compare_cells, random_tables
from test_resolve_cpu import CASES, SAFETY, gadget_inputs, golden_trees, opponents_best_response, order_check, safety_game

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def arm(solver, P, alt, regret, ssum):
    solver.set_gadget(P, alt)
    zr, zs = solver.gadget()
    assert not zr.any() and not zs.any() and zr.shape == (2, len(alt))            # set_gadget zeroes the rows
    solver.set_gadget_rows(regret, ssum)
    gr, gs = solver.gadget()
    assert gr.tobytes() == regret.tobytes() and gs.tobytes() == ssum.tobytes()


def compare_gadget(game, P, p, before, got, want, what):
    """the gadget's cells after one sweep of traverser p -> (cells, cells that differ at all)"""
    if p == P:                                                                     # the resolver's sweep leaves them
        assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes(), (what, "the resolver's sweep wrote the gadget rows")
        return 0, 0
    used = (~game.blocked[1 - P]).any(axis=0)
    cells = differ = 0
    for g, w, b in zip(got, want, before):
        assert g[:, ~used].tobytes() == b[:, ~used].tobytes(), (what, "a hand without a dealt lane changed")
        d, _ = compare_cells(g[:, used], w[:, used], what)
        cells += d.size
        differ += int((d > 0).sum())
    return cells, differ


@pytest.mark.parametrize("name", CASES)
def test_one_gadget_sweep_equals_the_restatement(name):
    """both resolvers, both traversers, plain and RM+, rank-order and pair-loop leaves, random gadget rows (every third hand all non-positive) and alt with negative,
    zero and 1e30 entries: tables, gadget rows and value"""
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    c0, d0 = order_check(name, nodes, cids, sizes, game)                           # check (e) first: the restatement's two orders alone stay inside the cap
    assert d0 <= 0.005 * c0, (name, d0, c0)
    dev = Device(board0, h, cids, sizes, tree)
    cells = differ = 0
    for P in (0, 1):
        for p in (0, 1):
            for rmplus in (False, True):
                rng = np.random.Generator(np.random.PCG64(200 + 4 * P + 2 * p + rmplus))
                before = random_tables(rng, nodes, sizes)
                alt, gr, gs = gadget_inputs(rng, game.n[1 - P])
                want = copy_tables(*before)
                G = dict(resolver=P, alt=alt, regret=gr.copy(), ssum=gs.copy())
                value = nr.gadget_sweep(nodes, want[0], want[1], G, game, cids, p, rmplus)
                for sorted_showdowns in (True, False):
                    what = (name, P, p, rmplus, sorted_showdowns)
                    s = dev.solver(rmplus, sorted_showdowns)
                    dev.upload(*before)
                    arm(s, P, alt, gr, gs)
                    got_value = s.iterate(p)
                    got, got_rows = dev.download(), s.gadget()
                    print(what, "value", got_value, "restated", value)
                    assert np.isclose(got_value, value, rtol=RTOL, atol=ATOL), (what, got_value, value)
                    c, d, _ = compare_sweep(nodes, game, cids, p, before, got, want, what)
                    cg, dg = compare_gadget(game, P, p, (gr, gs), got_rows, (G["regret"], G["ssum"]), what)
                    cells, differ = cells + c + cg, differ + d + dg
                    if name == "turn_no_opponent" and P == 1 and p == 0:           # hands 0 and 1 of player 0 meet no opponent: S = 0, the regrets move by +0.0 only
                        moved = np.where(gr[:, :2] > 0, gr[:, :2], np.float32(0.0)) if rmplus else gr[:, :2]   # (RM+: a result that is not > 0 becomes 0)
                        assert (got_rows[0][:, :2] == moved).all(), what
                    if sorted_showdowns:                                           # determinism: the same call from the same state
                        dev.upload(*before)
                        arm(s, P, alt, gr, gs)
                        assert s.iterate(p) == got_value
                        again = s.gadget()
                        assert same_tables(dev.download(), got) and again[0].tobytes() == got_rows[0].tobytes() and again[1].tobytes() == got_rows[1].tobytes(), what
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    dev.close()


@pytest.mark.parametrize("name", ["turn_imperfect_recall", "river_lanes"])
def test_level_plan_and_depth_first_walk_give_the_same_bits_with_a_gadget(name):
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(221))
    before = random_tables(rng, nodes, sizes)
    for P in (0, 1):
        alt, gr, gs = gadget_inputs(rng, len(h[1 - P]))
        for rmplus in (False, True):
            for sorted_showdowns in (True, False):
                dev.upload(*before)
                levels = dev.solver(rmplus, sorted_showdowns)
                arm(levels, P, alt, gr, gs)
                v = [levels.iterate(0), levels.iterate(1)]
                assert levels.launches() > 0
                got, rows = dev.download(), levels.gadget()
                with depth_first():
                    walk = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns)
                    dev.upload(*before)
                    arm(walk, P, alt, gr, gs)
                    w = [walk.iterate(0), walk.iterate(1)]
                    assert walk.launches() == -1
                    wrows = walk.gadget()
                assert v == w, (name, P, rmplus, sorted_showdowns, v, w)
                assert same_tables(dev.download(), got) and rows[0].tobytes() == wrows[0].tobytes() and rows[1].tobytes() == wrows[1].tobytes(), (name, P, rmplus, sorted_showdowns)
                walk.destroy()
    dev.close()


def test_train_with_dcfr_equals_sweeps_and_ticks_issued_one_by_one_gadget_rows_included():
    """3 iterations with DCFR (1.5, 0, 2) against the same sweeps with the table's tick (rs_discount_dcfr) and the gadget's (one f32 multiply per cell, done here)"""
    board0, h, cids, sizes, tree = make_case("turn_lanes")
    nodes, _ = npr.build_tree(n_board_cards=4, bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(231))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = gadget_inputs(rng, len(h[0]))
    alt = np.where(alt > 1e29, 3.0, alt)                                           # (finite ticks: no inf * 0)
    for rmplus in (False, True):
        s = dev.solver(rmplus)
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        values = s.train(3, dcfr=True)
        whole, whole_rows = dev.download(), s.gadget()
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        for t in (1, 2, 3):
            one = [s.iterate(0), s.iterate(1)]
            f = rs.dcfr_factors(1.5, 0.0, 2.0, t)
            dev.table.discount_dcfr(*f)
            G = dict(zip(("regret", "ssum"), s.gadget()))
            nr.gadget_discount(G, *f)
            s.set_gadget_rows(G["regret"], G["ssum"])
        rows = s.gadget()
        assert same_tables(dev.download(), whole) and one == values.tolist()
        assert rows[0].tobytes() == whole_rows[0].tobytes() and rows[1].tobytes() == whole_rows[1].tobytes()
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        s.train(3)
        assert s.gadget()[1].tobytes() != whole_rows[1].tobytes()                  # the ticks did something to the gadget rows
    dev.close()


@pytest.mark.parametrize("name", ["river_lanes", "turn_imperfect_recall"])
def test_a_gadget_that_always_follows_is_no_gadget(name):
    """gadget_set to regret = (0, 1): the resolver's sweep equals the same object's sweep before set_gadget, bit for bit"""
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    rng = np.random.Generator(np.random.PCG64(241))
    before = random_tables(rng, nodes, sizes)
    for P in (0, 1):
        for rmplus in (False, True):
            dev = Device(board0, h, cids, sizes, tree)                             # a fresh object: it has not seen set_gadget
            s = dev.solver(rmplus)
            dev.upload(*before)
            plain = s.iterate(P)
            want = dev.download()
            n = len(h[1 - P])
            alt, _, gs = gadget_inputs(rng, n)
            arm(s, P, alt, np.stack([np.zeros(n), np.ones(n)]).astype(np.float32), gs)
            dev.upload(*before)
            assert s.iterate(P) == plain
            assert same_tables(dev.download(), want), (name, P, rmplus)
            dev.close()


def test_resolve_end_to_end_is_safe_and_equals_the_restatement():
    """test_resolve_cpu's safety run through rs.resolve.prepare / RangeCFR / graft / best_response_rounds: the device's best-response values of the opponent, before and
    after the graft, equal the restatement's to rtol 1e-6 (the bound test_deal_trainer_trains_full_width_on_its_own_game uses for trained values), and the grafted one is
    not above the trunk's."""
    board0, h, cids, sizes, tree, nodes, game = safety_game()
    P, O = SAFETY["resolver"], 1 - SAFETY["resolver"]
    # the restatement
    R, S = nrc.zero_tables(nodes, sizes)
    nrc.train(nodes, R, S, game, cids, SAFETY["trunk_iterations"])
    want_before = opponents_best_response(nodes, S, game, cids, P)
    pre = nr.prepare(nodes, (R, S), board0, h, cids, SAFETY["node"], SAFETY["prefix"], P, game=game)
    Rs, Ss = nrc.zero_tables(pre["nodes"], sizes)
    nr.gadget_train(pre["nodes"], Rs, Ss, nr.new_gadget(P, pre["alt"]), nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint"), pre["clusters"],
                    SAFETY["iterations"])
    grafted = copy_tables(R, S)
    nr.graft((Rs, Ss), grafted, pre, P)
    want_after = opponents_best_response(nodes, grafted[1], game, cids, P)
    # the device
    dev = Device(board0, h, cids, sizes, tree)
    br = lambda: dev.table.best_response_rounds(dev.tree, board0, h[0], h[1], cids, L.BR_MAX | L.BR_SORTED, deal="joint")[O]
    trunk = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, deal="joint")
    trunk.train(SAFETY["trunk_iterations"])
    got_before = br()
    prepared = resolve.prepare(dev.table, dev.tree, board0, h, cids, SAFETY["node"], SAFETY["prefix"], P, deal="joint")
    assert (prepared.node_map == pre["node_map"]).all() and (prepared.index_map == pre["index_map"]).all() and prepared.board.tolist() == pre["board"]
    assert all((prepared.hands[p] == pre["hands"][p]).all() and np.allclose(prepared.weights[p], pre["weights"][p], rtol=1e-6, atol=0) for p in (0, 1))
    assert np.allclose(prepared.alt, pre["alt"], rtol=1e-6, atol=1e-9)
    sub_table = rs.create_infosets(prepared.tree.n_action_nodes, prepared.tree, sizes[prepared.round0:], [1] * len(prepared.clusters), dtype=L.F32)
    solver = rs.RangeCFR(sub_table, prepared.tree, prepared.board, prepared.hands[0], prepared.hands[1], prepared.clusters, weights=prepared.weights, deal="joint")
    solver.set_gadget(P, prepared.alt)
    solver.train(SAFETY["iterations"])
    kept = {nd.index: dev.table.download_node(nd.index) for nd in dev.tree.action_nodes()}
    resolve.graft(sub_table, dev.table, prepared, P)
    got_after = br()
    print("opponent's best response: device", got_before, "->", got_after, "restated", want_before, "->", want_after)
    for nd in dev.tree.action_nodes():                                             # the graft wrote the resolver's rows below the node, nothing else
        now = dev.table.download_node(nd.index)
        inside = nd.index in prepared.index_map and nd.player == P
        assert inside or (now[0].tobytes() == kept[nd.index][0].tobytes() and now[1].tobytes() == kept[nd.index][1].tobytes()), nd.index
    assert np.isclose(got_before, want_before, rtol=1e-6, atol=0) and np.isclose(got_after, want_after, rtol=1e-6, atol=0), (got_before, want_before, got_after, want_after)
    assert got_after <= got_before
    solver.destroy()
    trunk.destroy()
    dev.close()


def as_dicts(tree):
    kinds = {L.NODE_PRIVATE_CHANCE: "private_chance", L.NODE_PUBLIC_CHANCE: "public_chance", L.NODE_ACTION: "action", L.NODE_TERMINAL: "terminal"}
    acts = {L.ACT_BET: "bet", L.ACT_RAISE: "raise", L.ACT_CHECK: "check", L.ACT_CALL: "call", L.ACT_FOLD: "fold"}
    terms = {L.TERM_ALLIN: "ALLIN", L.TERM_SHOWDOWN: "SHOWDOWN", L.TERM_UNCONTESTED: "UNCONTESTED"}
    out = []
    for nd in tree.nodes:
        d = dict(parent=nd.parent, children=[nd.children[k] for k in range(nd.n_children)], kind=kinds[nd.kind])
        if nd.kind == L.NODE_ACTION:
            d.update(player=nd.player, index=nd.index, round_idx=nd.round_idx, actions=[[acts[nd.action_kind[k]], nd.action_amt[k]] for k in range(nd.n_children)])
        elif nd.kind == L.NODE_TERMINAL:
            d.update(value=nd.value, ttype=terms[nd.ttype], last_to_act=nd.last_to_act, round=nd.round)
        elif nd.kind == L.NODE_PUBLIC_CHANCE:
            d.update(round=nd.round)
        out.append(d)
    return out


@pytest.mark.parametrize("name", ["river", "three_street"])
def test_subtree_equals_the_restated_cut_and_is_adopted(name):
    want_nodes = golden_trees()[name]
    _, tree = rs.build_game_tree(rs.default_flop() if name == "river" else rs.three_street_options())
    trunk = as_dicts(tree)
    assert len(trunk) == len(want_nodes)
    picked = [i for i, nd in enumerate(trunk) if nd["kind"] == "action"]
    if name == "three_street":
        picked = picked[:40] + picked[40::23]                                      # the first street's nodes and a spread of the later ones
    for node in picked:
        sub, node_map = tree.subtree(node)
        want, want_map = nr.cut(trunk, node)
        assert (node_map == want_map).all() and node_map.dtype == np.int32
        got = as_dicts(sub)
        for g, w in zip(got, want):
            assert all(g[k] == w[k] for k in g if k != "actions") and [list(a) for a in g.get("actions", [])] == [list(a) for a in w.get("actions", [])], (node, g, w)
        assert len(got) == len(want) and sub.n_action_nodes == sum(nd["kind"] == "action" for nd in want)
        again = rs.tree_from_nodes(sub.nodes)                                      # rs_tree_from_nodes adopts it
        assert again.n_nodes == sub.n_nodes and again.n_action_nodes == sub.n_action_nodes
    first = picked[0]
    sub, node_map = tree.subtree(first)
    assert (node_map == np.arange(first, tree.n_nodes)).all()


def test_refused_calls_leave_the_table_and_the_rows_alone():
    board0, h, cids, sizes, tree = make_case("river_lanes")
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(251))
    before = random_tables(rng, nodes, sizes)
    dev.upload(*before)
    kept = dev.download()
    s = dev.solver()
    with pytest.raises(rs.RsError) as e:                                           # gadget_get before set_gadget
        s.gadget()
    assert e.value.code == L.ERR_INVALID
    h_ = s._handle(None)
    assert L.load().rs_range_cfr_gadget_set(h_, None, None) == L.ERR_INVALID
    alt, gr, gs = gadget_inputs(rng, len(h[1]))
    with pytest.raises(rs.RsError) as e:                                           # bad resolver, on an object without a gadget: it stays without one
        s.set_gadget(2, alt)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(rs.RsError):
        s.gadget()
    arm(s, 0, alt, gr, gs)
    for bad in (np.nan, np.inf, -np.inf):                                          # a refused re-arming leaves alt and the rows
        poisoned = alt.copy()
        poisoned[-1] = bad
        with pytest.raises(rs.RsError) as e:
            s.set_gadget(0, poisoned)
        assert e.value.code == L.ERR_INVALID
    assert L.load().rs_range_cfr_set_gadget(h_, -1, alt.ctypes.data) == L.ERR_INVALID
    rows = s.gadget()
    assert rows[0].tobytes() == gr.tobytes() and rows[1].tobytes() == gs.tobytes()
    with pytest.raises(rs.RsError) as e:                                           # rs_tree_subtree on a terminal, a chance node, an id out of range
        dev.tree.subtree(next(i for i, nd in enumerate(dev.tree.nodes) if nd.kind == L.NODE_TERMINAL))
    assert e.value.code == L.ERR_INVALID
    for node in (0, -1, dev.tree.n_nodes):
        with pytest.raises(rs.RsError) as e:
            dev.tree.subtree(node)
        assert e.value.code == L.ERR_INVALID
    assert same_tables(dev.download(), kept)
    want = copy_tables(*before)                                                    # the refused calls changed nothing: the next sweep is the restatement's
    G = dict(resolver=0, alt=alt, regret=gr.copy(), ssum=gs.copy())
    value = nr.gadget_sweep(nodes, want[0], want[1], G, nbr.Game(board0, h), cids, 1)
    assert np.isclose(s.iterate(1), value, rtol=RTOL, atol=ATOL)
    dev.close()


def test_an_object_without_a_gadget_reports_the_launches_and_bytes_it_reported():
    """turn_imperfect_recall, rank-order showdowns, under the level plan.  The parent commit (no gadget in the library) reported launches() = 17 after
    iterate(0) and 17 after iterate(1), and nbytes = 779 336 after both, for this object; a gadget adds two launches per sweep (reach and TERMINATE leaf, or mass row
    and the gadget's own node) and its rows' bytes, and only to the object it is armed on."""
    board0, h, cids, sizes, tree = make_case("turn_imperfect_recall")
    dev = Device(board0, h, cids, sizes, tree)
    s = dev.solver()
    launches = []
    for p in (0, 1):
        s.iterate(p)
        launches.append(s.launches())
    print("launches", launches, "nbytes", s.nbytes)
    assert (tuple(launches), s.nbytes) == (PARENT_LAUNCHES, PARENT_BYTES)
    s.set_gadget(0, np.zeros(len(h[1])))
    for p in (0, 1):
        s.iterate(p)
        assert s.launches() == PARENT_LAUNCHES[p] + 2
    assert s.nbytes > PARENT_BYTES
    dev.close()


PARENT_LAUNCHES, PARENT_BYTES = (17, 17), 779336   # measured on the parent commit, one MI355X
