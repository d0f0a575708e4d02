"""GPU (-m gpu): the best response in the REAL game (RS_BR_MAX | RS_BR_REAL) -- the traverser's info sets are (prefix of the round, its own two cards), the opponent
still plays the abstracted average strategy.

The reference is the abstract machinery on an EXPANDED table: one cluster per (prefix, hand) pair for both players (ids f * n_p + h, test_np_br_cpu.lane_cids), its
strategy-sum columns gathered from the abstract table through the abstract ids (S_x[:, f * n_p + h] = S[:, cids[r][p][f, h]]), asked for plain RS_BR_MAX: the C oracle for
the bits (test_gpu_br_pinned.same: finite values by bits, NaN by NaN-ness), oracle/np_br.py through its sigma_bar callback within RTOL / ATOL of test_np_br_cpu.  Shapes are
the pinned tests': the smallest that still have prefix blocks, blocked lanes and tails.  Every tree here has own nodes whose child is an opponent's node (a bet is answered by
the other player), so the level plan's fold-in of those children is in every level-plan comparison.

Before the mode existed every call with the bit was refused with RS_ERR_INVALID ("mode is RS_BR_MAX or RS_BR_AVERAGE"), a message that does not name RS_BR_REAL: no test
of this file can pass there."""
import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from oracle import orc
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from test_gpu_br_pinned import GDT, NPDT, ODT, close, depth_first, edge_sums, plain_sums, python_cluster_ids, same
from test_np_br_cpu import FLOP, RIVER, TURN, exact_tie_game, lane_cids, pick_ranges, prefixes_of, random_cids, sizes_of

pytestmark = pytest.mark.gpu

REAL = L.BR_MAX | L.BR_REAL
PAIRS = ((REAL, L.BR_MAX), (REAL | L.BR_SORTED, L.BR_MAX | L.BR_SORTED))      # (device mode on the abstract table, oracle mode on the expanded one)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def real_case(board0, h, cids, bets, raises, dtype, make_sums, seed, sizes=None, with_np_br=True):
    """device on the abstract table with | BR_REAL against the oracle (and np_br) on the expanded table, level plan and depth first, pair loop and rank order; returns
    (real values, abstract values) of the pair-loop mode"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = sizes or sizes_of(cids)
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    table = rs.create_infosets(n_actions, tree, sizes, [1] * len(cids), dtype=GDT[dtype])
    ot = orc.OracleTree(orc.make_options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    lanes = lane_cids(board0, h)
    otab = orc.OracleDealTable(ot, [(pf * len(h[0]), pf * len(h[1])) for pf in prefixes_of(board0)], dtype=ODT[dtype])
    sums_x = {}
    for nd in tree.action_nodes():
        S = make_sums(rng, (nd.n_children, sizes[nd.round_idx][nd.player]), dtype, nd)
        table.upload_node(nd.index, np.zeros(S.shape, dtype=NPDT[dtype]), S)
        sums_x[nd.index] = np.ascontiguousarray(S[:, cids[nd.round_idx][nd.player].ravel()])
        otab.set_node(nd.index, np.zeros(sums_x[nd.index].shape), sums_x[nd.index])
    want = {dev: otab.best_response_rounds(board0, h[0], h[1], lanes, om) for dev, om in PAIRS}
    got = {}
    for dev, _ in PAIRS:
        got[dev] = table.best_response_rounds(tree, board0, h[0], h[1], cids, dev)
        print("level plan", hex(dev), got[dev], want[dev])
        same(got[dev], want[dev], ("level plan", dev))
    with depth_first():
        for dev, _ in PAIRS:
            same(table.best_response_rounds(tree, board0, h[0], h[1], cids, dev), want[dev], ("depth first", dev))
    if len(board0) == 5:     # the single-round entry point takes the same game
        same(table.best_response(tree, board0, h[0], cids[0][0][0], h[1], cids[0][1][0], REAL), want[REAL], "rs_best_response")
    if with_np_br:
        nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises)
        sig_x = {i: nbr.final_strategy(S) for i, S in sums_x.items()}
        ref = nbr.best_response(nodes, sig_x.__getitem__, board0, h, lanes, "max", None, nbr.Game(board0, h))
        for dev, _ in PAIRS:
            close(got[dev], ref, ("np_br", dev))
    absv = table.best_response_rounds(tree, board0, h[0], h[1], cids, L.BR_MAX)
    print("abstract", absv)
    return got[REAL], absv


def never_below(real, absv):
    assert (real >= absv - 1e-9 * np.abs(absv)).all(), (real, absv)


CASES = {
    # name: (board, hands of player 0 and 1, bet sizes and raise sizes per round, clusters per round, cell type, whether the gap to the abstract value is asserted)
    "river_wide_i32": (RIVER, 61, 47, ((0.5, 1.0),), ((3.0,),), [(6, 5)], "i32", False),
    "turn_f32": (TURN, 30, 26, ((0.5,),), ((),), [(6, 5), (9, 7)], "f32", True),
    "turn_wide_f16": (TURN, 30, 26, ((0.5, 1.0),), ((3.0,),), [(6, 5), (9, 7)], "f16", True),
    "flop_i32": (FLOP, 12, 15, ((0.5,),), ((),), [(4, 3), (6, 5), (9, 7)], "i32", True),
    "turn_one_hand_p0": (TURN, 1, 40, ((0.5,),), ((),), [(1, 4), (3, 5)], "i32", False),
    "turn_one_hand_p1": (TURN, 40, 1, ((0.5,),), ((),), [(4, 1), (3, 5)], "i32", False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_real_game_best_response_equals_the_oracle_on_the_expanded_table(name):
    """random (imperfect-recall) ids and random strategy sums: bits of the C oracle, np_br within rounding, and never below the abstract value (a response in the real game
    can copy any response of the abstracted one); on the turn and flop games the two differ by far more than rounding"""
    board0, n0, n1, bets, raises, clusters, dtype, gap = CASES[name]
    rounds = 6 - len(board0)
    rng = np.random.Generator(np.random.PCG64(len(name) + n0))
    h = pick_ranges(rng, board0, n0, n1)
    cids = random_cids(rng, board0, h, clusters)
    real, absv = real_case(board0, h, cids, bets * rounds, raises * rounds, dtype, lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype), n1, sizes=clusters)
    never_below(real, absv)
    if gap:
        assert real.sum() > absv.sum() + 1e-3, (real, absv)


@pytest.mark.parametrize("board0,n0,n1", [(RIVER, 61, 47), (TURN, 30, 26), (FLOP, 12, 15)], ids=["river", "turn", "flop"])
def test_identity_ids_make_the_two_modes_one(board0, n0, n1):
    """the abstract table itself with one cluster per (prefix, hand): BR_MAX | BR_REAL adds the same lanes in the same order as BR_MAX -- equal bits, no reference needed"""
    rounds = 6 - len(board0)
    rng = np.random.Generator(np.random.PCG64(n0 * n1))
    h = pick_ranges(rng, board0, n0, n1)
    lanes = lane_cids(board0, h)
    sizes = [(pf * n0, pf * n1) for pf in prefixes_of(board0)]
    wide = len(board0) > 3                                                  # (the flop's table has 2 352 x 15 columns per river node: the small tree there)
    bets, raises = (((0.5, 1.0),) if wide else ((0.5,),)) * rounds, (((3.0,),) if wide else ((),)) * rounds
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    table = rs.create_infosets(n_actions, tree, sizes, [1] * rounds, dtype=L.I32)
    for nd in tree.action_nodes():
        S = plain_sums(rng, (nd.n_children, sizes[nd.round_idx][nd.player]), "i32")
        table.upload_node(nd.index, np.zeros(S.shape, dtype=np.int32), S)
    for extra in (0, L.BR_SORTED):
        want = table.best_response_rounds(tree, board0, h[0], h[1], lanes, L.BR_MAX | extra)
        same(table.best_response_rounds(tree, board0, h[0], h[1], lanes, REAL | extra), want, ("level plan", extra))
        with depth_first():
            same(table.best_response_rounds(tree, board0, h[0], h[1], lanes, REAL | extra), want, ("depth first", extra))


def test_first_maximum_on_an_exact_tie_in_the_real_game():
    """test_np_br_cpu.exact_tie_game through the real-game form: bits of the oracle on the expanded table, which takes the first maximum (cfr.rs:684-690)"""
    board0, h, cids, bets, raises, nodes, sums = exact_tie_game()
    real, absv = real_case(board0, h, cids, bets, raises, "i32", lambda rng, shape, dtype, nd: sums[nd.index], 0, with_np_br=False)
    never_below(real, absv)


def test_nan_reach_stays_with_the_action_already_chosen():
    """the poisoned column of the pinned tests (+inf in action 0 of cluster 1 of player 1's first-round nodes, f32): as the opponent player 1 reaches with NaN, a NaN sum is
    never the smaller side of <, so out[0] is NaN; player 1 as the traverser never reads its own strategy: out[1] is finite.  NaN-ness as the oracle's"""
    rng = np.random.Generator(np.random.PCG64(11))
    h = pick_ranges(rng, TURN, 40, 37)
    cids = random_cids(rng, TURN, h, [(6, 5), (9, 7)])
    fill = lambda rng, shape, dtype, nd: edge_sums(rng, shape, dtype, poison=(nd.player == 1 and nd.round_idx == 0))
    real, _ = real_case(TURN, h, cids, ((0.5,),) * 2, ((),) * 2, "f32", fill, 9, sizes=[(6, 5), (9, 7)], with_np_br=False)
    assert np.isnan(real[0]) and np.isfinite(real[1]), real


def test_average_with_real_is_refused():
    h = pick_ranges(np.random.Generator(np.random.PCG64(2)), RIVER, 5, 6)
    cids = [[np.zeros((1, 5), dtype=np.uint32), np.zeros((1, 6), dtype=np.uint32)]]
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=5, bet_sizes=((0.5,),), raise_sizes=((),)))
    table = rs.create_infosets(n_actions, tree, [(1, 1)], [1], dtype=L.I32)
    for mode in (L.BR_AVERAGE | L.BR_REAL, L.BR_AVERAGE | L.BR_REAL | L.BR_SORTED):
        with pytest.raises(L.RsError) as e:
            table.best_response_rounds(tree, RIVER, h[0], h[1], cids, mode)
        assert e.value.code == L.ERR_INVALID and "RS_BR_REAL" in str(e.value)


# br_launches() of test_through_the_trainer's level plan after the abstract and after the real-game call, by showdown mode: host logic alone decides them, so they are
# exact.  Recorded on the GPU at commit afa54d2, before the level plan and the depth-first walk shared one job table and one launcher.
TRAINER_LAUNCHES = {0: (24, 23), L.BR_SORTED: (24, 23)}


def test_through_the_trainer():
    """a bucketed turn-start trainer (turn_bucketed_f32 of the pinned tests): the trainer's real-game call equals the table-level call with ids computed in Python,
    exploitability(real=True) is half its sum, the kept objects and their workspace serve both kinds of call (br_bytes does not move), the value follows the table"""
    rng = np.random.Generator(np.random.PCG64(57))
    mask = ab.card_mask("4d5dAs3c")
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.choice(len(allh), n, replace=False))] for n in (40, 31)]
    files = [(np.arange(13960050, dtype=np.uint64) * 2654435761 % 23).astype(np.uint32), None]       # a bucket file of the turn's index size
    bets, raises = ((0.5,),) * 2, ((),) * 2
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=bets, raise_sizes=raises))
    card_abs = [ab.CardAbstraction.init(ranges, mask, ab.TURN + r, files[r]) for r in range(2)]
    tr = rs.DealTrainer(tree, card_abs, ranges, mask, 1 << 12, seed=9, discount_interval=0, dtype=L.F32, prune_threshold=None, scale=0.5)
    board0, cids = python_cluster_ids(mask, ranges, card_abs, files)
    tr.train(3)
    tr.status()
    first = {}
    for extra in (0, L.BR_SORTED):
        absv = tr.best_response(L.BR_MAX | extra)
        assert tr.br_launches(bool(extra)) == TRAINER_LAUNCHES[extra][0]
        held = tr.br_bytes()
        first[extra] = tr.best_response(REAL | extra)
        assert tr.br_bytes() == held                                       # the workspace is shared
        assert tr.br_launches(bool(extra)) == TRAINER_LAUNCHES[extra][1]
        same(first[extra], tr.infosets.best_response_rounds(tree, board0, ranges[0], ranges[1], cids, REAL | extra), ("trainer against the table-level call", extra))
        never_below(first[extra], absv)
        assert tr.exploitability(sorted_showdowns=bool(extra), real=True) == first[extra].sum() / 2.0
        same(tr.best_response(L.BR_MAX | extra), absv, "the abstract call after a real one")
    with pytest.raises(L.RsError) as e:
        tr.best_response(L.BR_AVERAGE | L.BR_REAL)
    assert e.value.code == L.ERR_INVALID
    tr.train(5)
    tr.status()
    second = tr.best_response(REAL)
    assert second.tobytes() != first[0].tobytes()
    same(second, tr.infosets.best_response_rounds(tree, board0, ranges[0], ranges[1], cids, REAL), "after more training")
    tr.destroy()
