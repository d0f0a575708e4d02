"""CPU: weighted hand ranges.  The numpy restatement (tests/np_weighted.py: the dense deal tensor W[b][h0][h1] rebuilt from per-hand weights, for both deal
distributions) against what the two distributions are known to do; the wrapper's zero-weight dropping (rustsolver_amd.solver.drop_zero_weights); the new symbols.

  * W is a distribution; unit weights give np_br.Game's W bit for bit; doubling one player's weights and halving the other's changes no bit; the two distributions
    differ on unequal ranges;
  * integer weights k on player 1 ARE the range with each hand listed k times (cluster columns repeated), under "max" and "avg", in both distributions.
The cases (CASES, make_case, tables_of) are the ones tests/test_gpu_weighted.py runs on the device."""
import ctypes as C

import numpy as np
import pytest

import np_weighted as nw
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from rustsolver_amd import solver as sv
from test_np_br_cpu import ATOL, FLOP, RIVER, RTOL, TURN, check_margins, lane_cids, pick_ranges, random_cids, sizes_of
from test_range_cfr_cpu import random_tables

CASES = {
    # name: (board0, hands of player 0 and 1, clusters, bet sizes, raise sizes, seed)
    "RIVER": (RIVER, 40, 47, [(6, 9)], ((0.5, 1.0),), ((3.0,),), 101),
    "TURN": (TURN, 33, 41, [(7, 5), (9, 12)], ((0.5,), (1.0,)), ((), ()), 102),
    "FLOP": (FLOP, 12, 15, [(4, 3), (6, 5), (8, 7)], ((0.5,), (0.5,), (1.0,)), ((), (), ()), 103),
}


def make_case(name, lanes=False):
    """-> dict(board0, h, cids, sizes, tree=(bets, raises), nodes, w): ranges, random_cids (lanes: one info set per (prefix, hand) instead) and weights
    rng.integers(1, 9) / 4, drawn in that order from PCG64(seed)"""
    board0, n0, n1, clusters, bets, raises, seed = CASES[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    h = pick_ranges(rng, board0, n0, n1)
    cids = random_cids(rng, board0, h, clusters)
    w = [rng.integers(1, 9, n) / 4.0 for n in (n0, n1)]
    sizes = list(clusters)
    if lanes:
        cids = lane_cids(board0, h)
        sizes = sizes_of(cids)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises)
    return dict(board0=board0, h=h, cids=cids, sizes=sizes, tree=(bets, raises), nodes=nodes, w=w, seed=seed)


def tables_of(case, dtype="f32"):
    """(R, S) per action node from PCG64(seed + 1000): f32 as test_range_cfr_cpu.random_tables, i32 regrets in [-1000, 1000) and sums in [0, 1000) with 15 % zeros"""
    rng = np.random.Generator(np.random.PCG64(case["seed"] + 1000))
    R, S = random_tables(rng, case["nodes"], case["sizes"])
    if dtype == "i32":
        for i in R:
            R[i] = rng.integers(-1000, 1000, R[i].shape).astype(np.int32)
            s = rng.integers(0, 1000, S[i].shape)
            s[rng.random(S[i].shape) < 0.15] = 0
            S[i] = s.astype(np.int32)
    return R, S


def strategies_of(tables, current=False, dtype="f32"):
    R, S = tables
    if not current:
        return {i: nbr.final_strategy(S[i]) for i in S}
    return {i: (npr.get_strategy(R[i]) if dtype == "i32" else npr.get_strategy_f32(R[i])) for i in R}


def game_of(case, deal, weights="case"):
    return nw.WeightedGame(case["board0"], case["h"], case["w"] if weights == "case" else weights, deal)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restated_deal_tensor(name):
    case = make_case(name)
    plain = nbr.Game(case["board0"], case["h"])
    for deal in nw.DEALS:
        g = game_of(case, deal)
        assert abs(g.W.sum() - 1.0) < 1e-12, (name, deal, g.W.sum())
        assert ((g.W > 0) == (plain.W > 0)).all()
        twice = game_of(case, deal, (case["w"][0] * 2.0, case["w"][1] * 0.5))
        assert twice.W.tobytes() == g.W.tobytes(), (name, deal)
        other = game_of(case, deal, (case["w"][0] * 0.5, case["w"][1] * 2.0))
        assert other.W.tobytes() == g.W.tobytes(), (name, deal)
    for weights in ((None, None), (np.ones(len(case["h"][0])), None), (None, np.ones(len(case["h"][1])))):
        assert game_of(case, "sequential", weights).W.tobytes() == plain.W.tobytes(), name
    # unequal ranges: N0(b) N1(b, h0) varies with the lane, so the two distributions differ even at unit weights -- and with weights
    assert not np.allclose(game_of(case, "joint", (None, None)).W, plain.W, rtol=1e-6, atol=0)
    assert not np.allclose(game_of(case, "joint").W, game_of(case, "sequential").W, rtol=1e-6, atol=0)
    assert not np.allclose(game_of(case, "sequential").W, plain.W, rtol=1e-6, atol=0)


def test_joint_is_the_product_of_the_ranges_with_card_removal():
    """P(b, h0, h1) proportional to W0[h0] W1[h1] over the deals, straight from the definition (no Z1, no lanes)"""
    case = make_case("TURN")
    g = game_of(case, "joint")
    raw = np.where(nbr.Game(case["board0"], case["h"]).W > 0, case["w"][0][None, :, None] * case["w"][1][None, None, :], 0.0)
    assert np.allclose(g.W, raw / raw.sum(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("deal", nw.DEALS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_weights_are_repeated_hands(name, deal):
    """k copies of a hand of player 1 = the hand with weight k: np_br on the WeightedGame against np_br on the unit-weight game of the longer range"""
    case = make_case(name)
    k = np.random.Generator(np.random.PCG64(case["seed"] + 7)).integers(1, 4, len(case["h"][1]))
    assert k.max() > 1
    sig = strategies_of(tables_of(case, "i32"), dtype="i32")
    weighted = game_of(case, deal, (None, k.astype(np.float64)))
    hands, cids = nw.repeat_hands(case["h"], case["cids"], 1, k)
    listed = nw.WeightedGame(case["board0"], hands, (None, None), deal)
    if deal == "sequential":
        assert listed.W.tobytes() == nbr.Game(case["board0"], hands).W.tobytes()
    for mode in ("max", "avg"):
        margins = [] if mode == "max" else None
        a = nbr.best_response(case["nodes"], sig.__getitem__, None, None, case["cids"], mode, margins, weighted)
        b = nbr.best_response(case["nodes"], sig.__getitem__, None, None, cids, mode, None, listed)
        assert np.allclose(a, b, rtol=RTOL, atol=ATOL), (name, deal, mode, a, b)
        if margins is not None:
            check_margins(margins)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cases_argmax_margins_are_clear_of_rounding(name):
    """what tests/test_gpu_weighted.py asserts again before it compares BR_MAX: every table type, both distributions, average and current strategies"""
    case = make_case(name)
    for dtype in ("i32", "f32"):
        for current in (False, True):
            sig = strategies_of(tables_of(case, dtype), current, dtype)
            for deal in nw.DEALS:
                margins = []
                nbr.best_response(case["nodes"], sig.__getitem__, None, None, case["cids"], "max", margins, game_of(case, deal))
                print(name, dtype, current, deal, "smallest relative margin", check_margins(margins))


def test_drop_zero_weights():
    case = make_case("TURN")
    h, cids = case["h"], case["cids"]
    w0 = case["w"][0].copy()
    w0[[0, 7, 32]] = 0.0
    hands, cl, w, keep = sv.drop_zero_weights(h, cids, (w0, None))
    assert keep[1] is None and w[1] is None and keep[0].tolist() == (w0 != 0).tolist() and keep[0].sum() == 30
    assert (hands[0] == h[0][keep[0]]).all() and (hands[1] == h[1]).all() and hands[0].dtype == np.uint8 and hands[0].flags.c_contiguous
    assert w[0].tolist() == w0[keep[0]].tolist() and w[0].dtype == np.float64 and w[0].flags.c_contiguous
    for r in range(len(cids)):
        assert cl[r][0].shape == (cids[r][0].shape[0], 30) and (cl[r][0] == cids[r][0][:, keep[0]]).all() and cl[r][0].flags.c_contiguous
        assert (cl[r][1] == cids[r][1]).all() and cl[r][0].dtype == np.uint32
    # nothing to drop: everything as given; other bad weights stay for the library to refuse
    hands, cl, w, keep = sv.drop_zero_weights(h, cids, (None, case["w"][1]))
    assert keep[0] is None and keep[1].all() and all((cl[r][p] == cids[r][p]).all() for r in range(len(cids)) for p in (0, 1))
    hands, cl, w, keep = sv.drop_zero_weights(h, cids, None)
    assert w == [None, None] and keep == [None, None] and (hands[0] == h[0]).all()
    bad = case["w"][1].copy()
    bad[3], bad[4] = -1.0, np.nan
    hands, cl, w, keep = sv.drop_zero_weights(h, cids, (None, bad))
    assert keep[1].all() and w[1][3] == -1.0 and np.isnan(w[1][4])
    with pytest.raises(ValueError):
        sv.drop_zero_weights(h, cids, (w0[:-1], None))
    # flat cluster tables of a one-prefix round
    flat = [[cids[0][0].reshape(-1), cids[0][1].reshape(-1)]]
    _, cl, _, _ = sv.drop_zero_weights(h, flat, (w0, None))
    assert cl[0][0].reshape(-1).tolist() == cids[0][0][0, w0 != 0].tolist()
    # the columns come back as zeros in a report's rows
    block = dict(cfv=np.ones((2, 3, 30)), value=np.ones((3, 30)))
    full = sv._restore_columns({5: block}, w0 != 0)[5]
    assert full["cfv"].shape == (2, 3, 33) and (full["cfv"][..., [0, 7, 32]] == 0).all() and full["cfv"].sum() == 2 * 3 * 30 and full["value"].shape == (3, 33)


def test_the_new_symbols_are_bound():
    lib = L.load()
    for name in ("rs_best_response_weighted", "rs_node_report_weighted", "rs_range_cfr_create_weighted"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert (L.DEAL_SEQUENTIAL, L.DEAL_JOINT) == (0, 1)
    assert C.sizeof(L.RangeWeights) == 2 * C.sizeof(C.c_void_p) + 8
    assert [f[0] for f in L.RangeWeights._fields_] == ["w", "deal", "reserved"]
    # refused on the host, before any device is touched: no GPU needed
    w = np.array([1.0, 0.0])
    rw = L.RangeWeights()
    rw.w[0], rw.deal = w.ctypes.data, L.DEAL_SEQUENTIAL
    out = np.full(2, 7.0)
    dummy = np.zeros(8, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rs_best_response_weighted(vp(dummy), vp(dummy), vp(dummy), 5, vp(dummy), 2, vp(dummy), 2, vp(dummy), 1, C.byref(rw), L.BR_MAX,
                                         out.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_INVALID
    assert b"rs_range_weights" in lib.rs_last_error() and (out == 7.0).all()
