"""CPU: rake (rs_rake) -- rs_rake_payoffs against the header's formulas, and the numpy restatement tests/np_rake.py against the identities the definition implies, on the
cases tests/test_gpu_rake.py holds the device to.

  * rs_rake_payoffs on every terminal of the river, turn and flop trees, both players, both sides of the cap, folder and non-folder; its refusals leave `out` alone;
  * without rake np_rake is np_locks / np_br to the bit;
  * conservation: the two players' raked average values add up to minus the expected rake, which an independent walk computes (np_rake.expected_rake: every terminal an
    uncontested-style leaf of value r(n) on both reaches); unraked they add up to 0;
  * on a board that ties every deal, a showdown leaf is -r / 2 times the fold leaf of the same reach;
  * the second summation order (reverse=) agrees under rake;
  * the leaf kernels of rs_br.hip, raked and unraked, use no scratch and keep the occupancy the launcher's slice arithmetic assumes.
Rake everywhere: rate 0.05, cap 30, which caps pots above 600.  Only the default river tree has one (its pots are 35 to 1035: the all-in showdown of 1035 is capped,
every other terminal is not); the turn, flop and eight-action trees end at 315, 273 and 255, so under that rake alone they would never meet the cap.  Those cases run
under it all the same AND under a second rake of the same rate with cap 5 (pots above 100 are capped), so that every case has showdown leaves on both sides of a cap:
rakes_of, asserted where it is used.
f64 rows within RTOL, ATOL of test_np_br_cpu, table cells under test_range_cfr_cpu.compare_cells, at most 0.5 % of a case's cells differing at all.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import np_locks as nl
import np_node_report as nnr
import np_rake as nr
import np_weighted as nw
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_locks_cpu import random_locks
from test_node_report_cpu import close, rows_of, setup
from test_np_br_cpu import ATOL, RIVER, combos_of
from test_range_cfr_cpu import FLOP_TREE, RIVER_TREE, TURN_TREE, compare_cells, copy_of, make_shape, random_tables

RAKE = (0.05, 30.0)
LOW_CAP_RAKE = (0.05, 5.0)
CASES = ["river_wave_35", "turn_imperfect_recall", "flop_three_rounds", "river_eight_actions_thread"]   # test_gpu_locks.py's, and test_gpu_rake.py's
ALL_TIE_BOARD = [32, 37, 42, 47, 48]                                                # Ts Jh Qd Kc As, card = 4 * rank + suit: the board plays, every deal is a tie

_SETUPS = {}


def case(name):
    """test_node_report_cpu.setup's cases, and the 8-action river tree of test_range_cfr_cpu.make_shape the same way; built once and left unchanged"""
    if name != "river_eight_actions_thread":
        return setup(name)
    if name not in _SETUPS:
        board0, h, cids, sizes, tree = make_shape(name)
        nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
        tables = random_tables(np.random.Generator(np.random.PCG64(61)), nodes, sizes)
        _SETUPS[name] = dict(board0=board0, h=h, cids=cids, sizes=sizes, tree=tree, nodes=nodes, game=nbr.Game(board0, h), tables=tables)
    return _SETUPS[name]


def showdowns(nodes):
    return [nd for nd in nodes if nd["kind"] == "terminal" and nd["ttype"] != "UNCONTESTED"]


def both_sides_of_the_cap(nodes, rake=RAKE):
    """the tree has a showdown leaf whose rake is capped and one whose rake is not"""
    pots = [float(np.float32(nd["value"])) for nd in showdowns(nodes)]
    return any(rake[0] * x > rake[1] for x in pots) and any(rake[0] * x < rake[1] for x in pots)


def rakes_of(nodes):
    """RAKE, and LOW_CAP_RAKE as well where RAKE's cap lies above every showdown pot of the tree; between them showdown leaves on both sides of a cap"""
    rakes = [RAKE] if both_sides_of_the_cap(nodes) else [RAKE, LOW_CAP_RAKE]
    assert both_sides_of_the_cap(nodes, rakes[-1])
    return rakes


def formula(nd, rake, p):
    """the issue's table, written out once more: (win, tie, lose)"""
    pot = float(np.float32(nd["value"]))
    r = 0.0 if rake is None else min(rake[1], rake[0] * pot)
    if nd["ttype"] == "UNCONTESTED":
        return (-pot,) * 3 if p == nd["last_to_act"] else (pot - r,) * 3
    return pot - r, -0.5 * r, -pot


@pytest.mark.parametrize("n_board,tree", [(5, RIVER_TREE), (4, TURN_TREE), (3, FLOP_TREE)])
def test_payoffs_of_every_terminal_are_the_formulas(n_board, tree):
    import rustsolver_amd as rs
    from rustsolver_amd import rake as rk

    nodes, _ = npr.build_tree(n_board_cards=n_board, bet_sizes=tree[0], raise_sizes=tree[1])
    _, dev_tree = rs.build_game_tree(rs.Options(n_board_cards=n_board, bet_sizes=tree[0], raise_sizes=tree[1]))
    assert dev_tree.n_nodes == len(nodes)
    rakes = rakes_of(nodes)
    assert len(rakes) == (1 if n_board == 5 else 2)
    seen = set()
    for i, nd in enumerate(nodes):
        if nd["kind"] != "terminal":
            continue
        for p in (0, 1):
            for rake in (RAKE, LOW_CAP_RAKE, None, (0.05, np.inf), (1.0, 1e9), (0.0, 30.0), (0.05, 0.0)):
                got, want = rk.payoffs(dev_tree, i, rake, p), formula(nd, rake, p)
                assert got.tolist() == [float(x) for x in want], (i, p, rake, got, want)   # (-0.0 == 0.0)
                assert nr.payoffs(nd, rake, p) == tuple(got.tolist()), (i, p, rake)
            pot = float(np.float32(nd["value"]))
            seen.add((nd["ttype"] == "UNCONTESTED", p == nd["last_to_act"], rakes[-1][0] * pot > rakes[-1][1]))
            if nd["ttype"] == "UNCONTESTED":
                assert rk.payoffs(dev_tree, i, RAKE, p)[0] == (-pot if p == nd["last_to_act"] else pot - min(30.0, 0.05 * pot))
            else:
                assert rk.payoffs(dev_tree, i, None, p).tolist() == [pot, 0.0, -pot]
    assert {(True, True, False), (True, False, False), (False, True, True), (False, True, False), (False, False, True), (False, False, False)} <= seen
    if len(rakes) == 2:
        assert {(True, True, True), (True, False, True)} <= seen                    # a fold on the far side of the cap as well


def test_the_new_symbols_are_bound_and_payoffs_refuses():
    import rustsolver_amd as rs
    from rustsolver_amd import _lib as L
    from rustsolver_amd import rake as rk

    lib = L.load()
    for name in ("rs_rake_payoffs", "rs_best_response_raked", "rs_node_report_raked", "rs_range_cfr_create_raked"):
        assert name in L.SYMBOLS and getattr(lib, name) is not None
    assert C.sizeof(L.Rake) == 24
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=RIVER_TREE[0], raise_sizes=RIVER_TREE[1])
    _, tree = rs.build_game_tree(rs.Options(n_board_cards=5, bet_sizes=RIVER_TREE[0], raise_sizes=RIVER_TREE[1]))
    terminal = next(i for i, nd in enumerate(nodes) if nd["kind"] == "terminal")
    action = next(i for i, nd in enumerate(nodes) if nd["kind"] == "action")
    out = np.full(3, 7.0)

    def call(node, rake, player, tree_h=tree._h):
        p, _alive = rk.arg(rake)
        return lib.rs_rake_payoffs(tree_h, node, p, player, out.ctypes.data_as(C.POINTER(C.c_double)))

    refused = {"an action node": (action, RAKE, 0), "the deal": (0, RAKE, 0), "an id out of range": (len(nodes), RAKE, 0), "a negative id": (-1, RAKE, 0),
               "player 2": (terminal, RAKE, 2), "player -1": (terminal, None, -1),
               "a negative rate": (terminal, (-0.01, 30.0), 0), "a rate above 1": (terminal, (1.0 + 1e-9, 30.0), 0), "a NaN rate": (terminal, (np.nan, 30.0), 0),
               "an infinite rate": (terminal, (np.inf, 30.0), 0), "a NaN cap": (terminal, (0.05, np.nan), 0), "a negative cap": (terminal, (0.05, -1.0), 0),
               "a cap of -inf": (terminal, (0.05, -np.inf), 0), "reserved[0]": (terminal, (0.05, 30.0, (1, 0)), 0), "reserved[1]": (terminal, (0.05, 30.0, (0, -1)), 0)}
    for what, args in refused.items():
        assert call(*args) == L.ERR_INVALID, what
        assert lib.rs_last_error().startswith(b"rs_rake"), (what, lib.rs_last_error())
        assert (out == 7.0).all(), what
    assert call(terminal, RAKE, 0, None) == L.ERR_INVALID and (out == 7.0).all()
    assert call(terminal, RAKE, 0) == L.OK and not (out == 7.0).any()
    with pytest.raises(rs.RsError):
        rk.payoffs(tree, action, RAKE, 0)
    assert rk.paid([-3.0, 1.0]) == 2.0 and rk.exploitability([2.0, 1.0], [-3.0, 1.0]) == 2.5
    assert rk.exploitability([2.0, 1.0], [0.5, -0.5]) == 1.5                        # zero-sum averages: (max0 + max1) / 2


@pytest.mark.parametrize("rake", [None, (0.0, 30.0), (0.05, 0.0)])
def test_without_rake_the_restatement_is_np_locks_to_the_bit(rake):
    name = "turn_imperfect_recall"
    s = case(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    sig = nnr.strategies(s["tables"])
    locks = random_locks(name)
    for lk in (None, locks):
        for mode in ("max", "avg"):
            assert nr.best_response(nodes, sig.__getitem__, game, cids, mode, lk, rake=rake).tobytes() == nl.best_response(nodes, sig.__getitem__, game, cids, mode, lk).tobytes()
        assert (nr.best_response(nodes, sig.__getitem__, game, cids, "max", lk, real=True, rake=rake).tobytes()
                == nl.best_response(nodes, sig.__getitem__, game, cids, "max", lk, real=True).tobytes())
        for p in (0, 1):
            got, want = nr.report(nodes, sig.__getitem__, game, cids, p, lk, rake=rake), nl.report(nodes, sig.__getitem__, game, cids, p, lk)
            assert sorted(got) == sorted(want)
            assert all(x.tobytes() == y.tobytes() for k in want for (_, x), (_, y) in zip(rows_of(got[k]), rows_of(want[k])))
            A, B = copy_of(*s["tables"]), copy_of(*s["tables"])
            assert nr.sweep(nodes, A[0], A[1], game, cids, p, bool(p), lk, rake=rake) == nl.sweep(nodes, B[0], B[1], game, cids, p, bool(p), lk)
            assert all(A[t][k].tobytes() == B[t][k].tobytes() for t in (0, 1) for k in A[0])
    assert nl._Walk is not nr._RakedWalk                                            # the swap ends with the call
    want = nbr.best_response(nodes, sig.__getitem__, None, None, cids, "avg", None, game)
    assert nr.best_response(nodes, sig.__getitem__, game, cids, "avg", rake=rake).tobytes() == nl.best_response(nodes, sig.__getitem__, game, cids, "avg").tobytes()
    close(nr.best_response(nodes, sig.__getitem__, game, cids, "avg", rake=rake), want, "np_br")


@pytest.mark.parametrize("name", CASES + ["river_lanes", "turn_lanes"])
def test_the_two_raked_values_add_up_to_minus_the_expected_rake(name):
    s = case(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    for rake in rakes_of(nodes):
        for current in (False, True):
            sig = nnr.strategies(s["tables"], current)
            for lk in (None, random_locks(name) if name in ("turn_imperfect_recall", "flop_three_rounds") else None):
                avg = nr.best_response(nodes, sig.__getitem__, game, cids, "avg", lk, rake=rake)
                want = nr.expected_rake(nodes, sig.__getitem__, game, cids, rake, lk)
                print(name, rake, current, "avg", avg, "expected rake", want)
                assert want > 1.0                                                   # chips per deal: pots of 35 and more at 5 %
                close(avg[0] + avg[1], -want, (name, rake, current, "conservation"))
                free = nr.best_response(nodes, sig.__getitem__, game, cids, "avg", lk)
                assert abs(free[0] + free[1]) <= ATOL, (name, free)
                assert not np.allclose(avg, free, rtol=1e-6)
                mx = nr.best_response(nodes, sig.__getitem__, game, cids, "max", lk, rake=rake)
                assert (mx >= avg - 1e-9).all()
                e, paid = nr.exploitability(nodes, sig.__getitem__, game, cids, rake, lk)
                close(paid, want, (name, "paid"))
                assert e >= -1e-9


def all_tie_game(n0=24, n1=22, pool=30, seed=3):
    """both ranges drawn from one pool of combos of the all-tie board, so that many combos are in both"""
    rng = np.random.Generator(np.random.PCG64(seed))
    combos = combos_of(ALL_TIE_BOARD)
    pool = combos[np.sort(rng.choice(len(combos), pool, replace=False))]
    return [pool[np.sort(rng.choice(len(pool), n0, replace=False))], pool[np.sort(rng.choice(len(pool), n1, replace=False))]]


def in_both(h):
    a, b = ({tuple(sorted(x)) for x in np.asarray(r).tolist()} for r in h)
    return len(a & b)


def test_on_a_board_that_ties_every_deal_a_showdown_is_half_the_rake_times_the_fold_leaf():
    h = all_tie_game()
    assert in_both(h) >= 10
    game = nbr.Game(ALL_TIE_BOARD, h)
    assert (game.W > 0).sum() > 100 and (game.S[game.W > 0] == 0).all() and (game.S == 0).all()
    full = nbr.Game(ALL_TIE_BOARD, [combos_of(ALL_TIE_BOARD)[:30], combos_of(ALL_TIE_BOARD)[600:630]])
    assert (full.S == 0).all()
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=RIVER_TREE[0], raise_sizes=RIVER_TREE[1])
    rng = np.random.Generator(np.random.PCG64(11))
    seen = 0
    for reverse in (False, True):
        for p in (0, 1):
            w = nr._RakedWalk(nodes, game, None, p, None, reverse)
            w.rake = RAKE
            for nd in showdowns(nodes):
                q = rng.random((1, game.n[1 - p]))
                _, r = nr.rake_of(nd, RAKE)
                assert r > 0
                close(w.terminal(nd, q), -0.5 * r * w.leaf(w.M_fold, q), (p, reverse, nd["value"]))
                seen += 1
    assert seen >= 8


@pytest.mark.parametrize("name", CASES)
def test_the_reversed_summation_order_agrees_under_rake(name):
    s = case(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    cells = differ = 0
    for RK in rakes_of(nodes):
        for current in (False, True):
            sig = nnr.strategies(s["tables"], current)
            for mode in ("max", "avg"):
                close(nr.best_response(nodes, sig.__getitem__, game, cids, mode, rake=RK), nr.best_response(nodes, sig.__getitem__, game, cids, mode, reverse=True, rake=RK),
                      (name, mode, current))
            close(nr.best_response(nodes, sig.__getitem__, game, cids, "max", real=True, rake=RK),
                  nr.best_response(nodes, sig.__getitem__, game, cids, "max", real=True, reverse=True, rake=RK), (name, "real", current))
        sig = nnr.strategies(s["tables"])
        for p in (0, 1):
            fwd, rev = nr.report(nodes, sig.__getitem__, game, cids, p, rake=RK), nr.report(nodes, sig.__getitem__, game, cids, p, reverse=True, rake=RK)
            for k in fwd:
                for (row, x), (_, y) in zip(rows_of(fwd[k]), rows_of(rev[k])):
                    close(x, y, (name, p, k, row))
            for rmplus in (False, True):
                A, B = copy_of(*s["tables"]), copy_of(*s["tables"])
                close(nr.sweep(nodes, A[0], A[1], game, cids, p, rmplus, rake=RK), nr.sweep(nodes, B[0], B[1], game, cids, p, rmplus, reverse=True, rake=RK), (name, p, rmplus))
                for k in A[0]:
                    for t in (0, 1):
                        d, _ = compare_cells(A[t][k], B[t][k], (name, p, rmplus, k, t))
                        cells, differ = cells + d.size, differ + int((d > 0).sum())
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)


def test_rake_composes_with_weighted_ranges_in_the_restatement():
    s = case("turn_imperfect_recall")
    nodes, cids = s["nodes"], s["cids"]
    rng = np.random.Generator(np.random.PCG64(17))
    w = [rng.random(len(h)) + 0.5 for h in s["h"]]
    sig = nnr.strategies(s["tables"])
    for deal in ("sequential", "joint"):
        game = nw.WeightedGame(s["board0"], s["h"], w, deal)
        avg = nr.best_response(nodes, sig.__getitem__, game, cids, "avg", rake=RAKE)
        close(avg[0] + avg[1], -nr.expected_rake(nodes, sig.__getitem__, game, cids, RAKE), deal)


# ---- the leaf kernels' registers: no scratch, and the occupancy the launcher's slice arithmetic (two workgroups per CU at full ranges, four otherwise) stands on ------------
LOOP_WAVES = {(1, 4): 4, (2, 8): 4, (4, 16): 4, (6, 21): 2}                          # at least this many waves per SIMD, raked or not
PARENT_WAVES = {(1, 4): 7, (2, 8): 6, (4, 16): 4, (6, 21): 2}                        # the unraked forms before rake: no lower


def test_the_leaf_kernels_use_no_scratch_and_keep_their_occupancy(tmp_path):
    from rustsolver_amd import build as B

    hipcc = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    os.makedirs(os.path.join(B.HERE, "_build"), exist_ok=True)
    cmd = [hipcc] + B.FLAGS + ["-x", "hip", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "rs_br.hip"), "-o", str(tmp_path / "rs_br.dev.o")]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-2000:]
    found = {}
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", done.stdout, re.S):
        if "k_br_terminal" in m.group(1):
            found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    loops = {}
    for name, (scratch, waves) in found.items():
        assert scratch == 0, (name, scratch)
        lm = re.search(r"k_br_terminal_sorted_loopILi(\d+)ELi(\d+)ELb[01]ELb([01])E", name)
        if lm:
            loops[(int(lm.group(1)), int(lm.group(2)), lm.group(3) == "1")] = waves
    print(sorted(found.items()))
    assert sorted(loops) == sorted((h, c, r) for (h, c) in LOOP_WAVES for r in (False, True)), sorted(loops)
    for (h, c, raked), waves in loops.items():
        assert waves >= (LOOP_WAVES[(h, c)] if raked else PARENT_WAVES[(h, c)]), (h, c, raked, waves)
    for entry in ("k_br_terminal_sorted_jobsILb", "k_br_terminal_boards_jobsILb"):     # both tree orders launch these
        both = sorted(n for n in found if entry in n)
        assert len(both) == 2, (entry, both)                                        # raked and unraked
        assert all(found[n][1] >= 8 for n in both), (entry, [found[n] for n in both])
