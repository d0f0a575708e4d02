"""GPU (-m gpu): rake (rs_best_response_raked, rs_node_report_raked, rs_range_cfr_create_raked) against the numpy restatement tests/np_rake.py.

The cases are tests/test_gpu_locks.py's.  Rake: rate 0.05, cap 30; the trees that have no pot above the 600 that cap needs run under cap 5 as well
(test_rake_cpu.rakes_of), so every case has showdown leaves on both sides of a cap.  What the raked leaf kernels add to the unraked ones is the tie mass and the
opponent's hand of the traverser's own two cards inside it: a board that ties every deal, ranges that overlap, and the leaf loop's four forms with both players holding
the same combos are there for that.  f64 rows and values within RTOL, ATOL of test_np_br_cpu (test_node_report_cpu.close), table cells as
test_gpu_range_cfr.compare_sweep compares them, at most 0.5 % of a case's cells differing at all; tests/test_rake_cpu.py holds the restatement's own two summation
orders to the same numbers.
"""
import ctypes as C

import numpy as np
import pytest

import np_node_report as nnr
import np_range_cfr as nrc
import np_rake as nr
import np_weighted as nw
import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from rustsolver_amd import rake as rk
from test_gpu_br_pinned import depth_first
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, make_case, same_tables
from test_locks_cpu import pick_nodes, random_lock
from test_node_report_cpu import close, rows_of
from test_np_br_cpu import RIVER, combos_of, lane_cids, pick_ranges, random_cids, sizes_of
from test_rake_cpu import ALL_TIE_BOARD, CASES, RAKE, all_tie_game, both_sides_of_the_cap, case, in_both, rakes_of
from test_range_cfr_cpu import RIVER_TREE, random_tables

pytestmark = pytest.mark.gpu

MODES = {L.BR_MAX: dict(mode="max"), L.BR_AVERAGE: dict(mode="avg"), L.BR_MAX | L.BR_REAL: dict(mode="max", real=True)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def device_of(s):
    dev = Device(s["board0"], s["h"], s["cids"], s["sizes"], s["tree"])
    assert dev.tree.n_nodes == len(s["nodes"])
    dev.upload(*s["tables"])
    return dev


def br(dev, mode, rake, **kw):
    return dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, mode, rake=rake, **kw)


def report(dev, p, ids, rake, **kw):
    return dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, rake=rake, **kw)


def solver(dev, rake, rmplus=False, sorted_showdowns=True, **kw):
    return rs.RangeCFR(dev.table, dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns, rake=rake, **kw)


def action_ids(nodes):
    return [i for i, nd in enumerate(nodes) if nd["kind"] == "action"]


def report_rows(got):
    return np.concatenate([x.reshape(-1) for i in sorted(got) for _, x in rows_of(got[i])])


def check_best_responses(dev, s, sig, rake, what, game=None, **kw):
    """every mode, rank-order and pair-loop leaves, level plan and depth-first walk, against the restatement -> the raked RS_BR_AVERAGE values"""
    nodes, cids = s["nodes"], s["cids"]
    game = game or s["game"]
    avg = None
    for mode, args in MODES.items():
        want = nr.best_response(nodes, sig.__getitem__, game, cids, rake=rake, locks=kw.get("locks"), **args)
        for sorted_bit in (L.BR_SORTED, 0):
            got = br(dev, mode | sorted_bit, rake, **kw)
            print(what, "mode", hex(mode | sorted_bit), rake, got, want)
            close(got, want, (what, mode, sorted_bit, rake))
            with depth_first():
                walked = br(dev, mode | sorted_bit, rake, **kw)
            close(walked, want, (what, mode, sorted_bit, rake, "depth first"))
            if sorted_bit:
                assert walked.tobytes() == got.tobytes(), (what, mode, rake, "the two tree orders, by rank order")
        if mode == L.BR_AVERAGE:
            avg = want
    return avg


def check_reports(dev, s, sig, rake, what, game=None, walks=(False,), **kw):
    nodes, cids = s["nodes"], s["cids"]
    game = game or s["game"]
    ids = action_ids(nodes)
    for p in (0, 1):
        want = nr.report(nodes, sig.__getitem__, game, cids, p, rake=rake, locks=kw.get("locks"))
        for sorted_showdowns in (True, False):
            for walk in walks:
                if walk:
                    with depth_first():
                        got = report(dev, p, ids, rake, sorted_showdowns=sorted_showdowns, **kw)
                else:
                    got = report(dev, p, ids, rake, sorted_showdowns=sorted_showdowns, **kw)
                assert sorted(got) == sorted(want)
                for i in want:
                    for (row, x), (_, y) in zip(rows_of(got[i]), rows_of(want[i])):
                        close(x, y, (what, rake, p, sorted_showdowns, walk, i, row))


@pytest.mark.timeout(180)
@pytest.mark.parametrize("name", CASES + ["turn_slices_7_8"])                       # ... and 7 x 8 hands: the depth-first walk's leaf jobs lie at rows beyond the table's first
def test_raked_walks_equal_the_restatement(name):
    """best response in every mode, every node-report row and one full-width sweep per traverser under rake; once with weighted ranges and once around a lock.  Without
    the feature nothing here can run: the wrappers have no rake= and the library no _raked entry points"""
    s = case(name)
    dev = device_of(s)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    sig = nnr.strategies(s["tables"])
    free = nbr.best_response(nodes, sig.__getitem__, None, None, cids, "avg", None, game)
    cells = differ = 0
    rakes = rakes_of(nodes)
    assert both_sides_of_the_cap(nodes, rakes[-1])
    for rake in rakes:
        avg = check_best_responses(dev, s, sig, rake, name)
        assert not np.allclose(avg, free, rtol=1e-6)                                # the rake matters
        assert not np.allclose(br(dev, L.BR_AVERAGE | L.BR_SORTED, rake), br(dev, L.BR_AVERAGE | L.BR_SORTED, None), rtol=1e-6)
        check_reports(dev, s, sig, rake, name)
        for p in (0, 1):
            before = copy_tables(*s["tables"])
            want = copy_tables(*before)
            value = nr.sweep(nodes, want[0], want[1], game, cids, p, bool(p), rake=rake)   # plain for traverser 0, RM+ for traverser 1
            for sorted_showdowns in (True, False):
                dev.upload(*before)
                sv = solver(dev, rake, bool(p), sorted_showdowns)
                got_value = sv.iterate(p)
                got = dev.download()
                sv.destroy()
                close(got_value, value, (name, rake, p, sorted_showdowns, "sweep value"))
                c, d, _ = compare_sweep(nodes, game, cids, p, before, got, want, (name, rake, p, sorted_showdowns))
                cells, differ = cells + c, differ + d
        dev.upload(*s["tables"])
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    rake = rakes[-1]
    rng = np.random.Generator(np.random.PCG64(17))
    w = [rng.random(len(h)) + 0.5 for h in s["h"]]                                  # random weights, the joint deal
    weighted = nw.WeightedGame(s["board0"], s["h"], w, "joint")
    for mode, args in ((L.BR_AVERAGE | L.BR_SORTED, dict(mode="avg")), (L.BR_MAX, dict(mode="max"))):
        close(br(dev, mode, rake, weights=w, deal="joint"), nr.best_response(nodes, sig.__getitem__, weighted, cids, rake=rake, **args), (name, "weighted", mode))
    node = pick_nodes(nodes)[-1]                                                    # and a lock no table row can express
    locks = {node: random_lock(np.random.Generator(np.random.PCG64(9)), nodes, game, s["board0"], node, garbage=len(s["board0"]) < 5)}
    for mode, args in ((L.BR_AVERAGE, dict(mode="avg")), (L.BR_MAX | L.BR_SORTED, dict(mode="max"))):
        close(br(dev, mode, rake, locks=locks), nr.best_response(nodes, sig.__getitem__, game, cids, locks=locks, rake=rake, **args), (name, "locked", mode))
    want = nr.report(nodes, sig.__getitem__, game, cids, 0, locks, rake=rake)
    got = report(dev, 0, action_ids(nodes), rake, locks=locks)
    for i in want:
        for (row, x), (_, y) in zip(rows_of(got[i]), rows_of(want[i])):
            close(x, y, (name, "locked report", i, row))
    dev.close()


def tie_case(which):
    """river games whose ranges overlap: the board that ties every deal, and the standard river board (wins, losses and ties side by side)"""
    if which == "all_ties":
        board0, h = ALL_TIE_BOARD, all_tie_game()
    else:
        rng = np.random.Generator(np.random.PCG64(23))
        combos = combos_of(RIVER)
        pool = combos[np.sort(rng.choice(len(combos), 40, replace=False))]
        board0, h = RIVER, [pool[np.sort(rng.choice(40, 30, replace=False))], pool[np.sort(rng.choice(40, 28, replace=False))]]
    rng = np.random.Generator(np.random.PCG64(29))
    sizes = [(3, 4)]
    cids = random_cids(rng, board0, h, sizes)
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=RIVER_TREE[0], raise_sizes=RIVER_TREE[1])
    return dict(board0=board0, h=h, cids=cids, sizes=sizes, tree=RIVER_TREE, nodes=nodes, game=nbr.Game(board0, h), tables=random_tables(rng, nodes, sizes))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("which", ["all_ties", "mixed"])
def test_ties_and_the_hand_of_the_same_two_cards(which):
    s = tie_case(which)
    game = s["game"]
    assert in_both(s["h"]) >= 10
    dealt = game.W > 0
    if which == "all_ties":
        assert (game.S[dealt] == 0).all()
    else:
        assert (game.S[dealt] == 0).any() and (game.S[dealt] > 0).any() and (game.S[dealt] < 0).any()
    assert both_sides_of_the_cap(s["nodes"])
    dev = device_of(s)
    sig = nnr.strategies(s["tables"])
    check_best_responses(dev, s, sig, RAKE, which)                                  # pair loop, rank-order body (depth first), leaf loop (level plan)
    check_reports(dev, s, sig, RAKE, which, walks=(False, True))
    want = nr.expected_rake(s["nodes"], sig.__getitem__, game, s["cids"], RAKE)
    for mode in (L.BR_AVERAGE, L.BR_AVERAGE | L.BR_SORTED):
        avg = br(dev, mode, RAKE)
        close(rk.paid(avg), want, (which, mode, "the rake paid"))
        with depth_first():
            close(rk.paid(br(dev, mode, RAKE)), want, (which, mode, "the rake paid, depth first"))
    dev.close()


LOOP_TREE = (((1.0,),), ((),))                                                      # one bet size, no raise: the smallest river tree


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n_hands", [200, 300, 600, 1081])
def test_the_leaf_loops_four_forms(n_hands):
    """k_br_terminal_sorted_loop<1,4>, <2,8>, <4,16> and <6,21> (ranges up to 256, 512, 1 024 combos and beyond), both players holding the same combos -- every
    traverser hand meets the opponent's hand of its own two cards -- against the pair loop on the device and against the restatement"""
    combos = combos_of(RIVER)
    assert len(combos) == 1081
    rng = np.random.Generator(np.random.PCG64(31))
    pick = combos[np.sort(rng.choice(len(combos), n_hands, replace=False))]
    h = [pick, pick.copy()]
    cids = lane_cids(RIVER, h)
    sizes = sizes_of(cids)
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=LOOP_TREE[0], raise_sizes=LOOP_TREE[1])
    tables = random_tables(rng, nodes, sizes)
    game = nbr.Game(RIVER, h)
    dealt = game.W > 0
    assert (game.S[dealt] == 0).any() and (game.S[dealt] != 0).any()
    dev = Device(RIVER, h, cids, sizes, LOOP_TREE)
    dev.upload(*tables)
    sig = nnr.strategies(tables)
    rake = (0.05, 3.0)                                                              # this tree's showdown pots are 35 and 105: one on either side of this cap
    assert both_sides_of_the_cap(nodes, rake) and not both_sides_of_the_cap(nodes, RAKE)
    for rake in (RAKE, rake):
        for mode, args in ((L.BR_AVERAGE, dict(mode="avg")), (L.BR_MAX, dict(mode="max"))):
            want = nr.best_response(nodes, sig.__getitem__, game, cids, rake=rake, **args)
            loop, pairs = br(dev, mode | L.BR_SORTED, rake), br(dev, mode, rake)
            print(n_hands, rake, hex(mode), loop, pairs, want)
            close(loop, pairs, (n_hands, rake, mode, "leaf loop against pair loop"))
            close(loop, want, (n_hands, rake, mode, "leaf loop against the restatement"))
            close(pairs, want, (n_hands, rake, mode, "pair loop against the restatement"))
        assert not np.allclose(br(dev, L.BR_AVERAGE | L.BR_SORTED, rake), br(dev, L.BR_AVERAGE | L.BR_SORTED, None), rtol=1e-6)
    dev.close()


@pytest.mark.timeout(60)
def test_no_rake_is_the_call_without_the_argument():
    """rake=None, rate 0 and cap 0: the bytes of the call without rake=, the same launches and the same held bytes"""
    s = case("turn_imperfect_recall")
    dev = device_of(s)
    ids = action_ids(s["nodes"])
    modes = (L.BR_MAX, L.BR_AVERAGE | L.BR_SORTED, L.BR_MAX | L.BR_REAL | L.BR_SORTED)

    def everything(**kw):
        out = dict(br=[dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, m, **kw) for m in modes],
                   rep=[report_rows(dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, **kw)) for p in (0, 1)])
        dev.upload(*s["tables"])
        sv = rs.RangeCFR(dev.table, dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, **kw)
        out["held0"] = sv.nbytes
        out["values"] = [sv.iterate(0), sv.iterate(1)]
        out["launches"], out["held"] = sv.launches(), sv.nbytes
        out["tables"] = dev.download()
        sv.destroy()
        dev.upload(*s["tables"])
        return out

    def same(a, b):
        return (all(x.tobytes() == y.tobytes() for x, y in zip(a["br"] + a["rep"], b["br"] + b["rep"])) and a["values"] == b["values"] and same_tables(a["tables"], b["tables"])
                and (a["launches"], a["held0"], a["held"]) == (b["launches"], b["held0"], b["held"]))

    plain = everything()
    assert plain["launches"] > 0
    for rake in (None, (0.0, 30.0), (0.05, 0.0)):
        assert same(everything(rake=rake), plain), rake
    raked = everything(rake=RAKE)
    assert not same(raked, plain)
    assert (raked["launches"], raked["held0"], raked["held"]) == (plain["launches"], plain["held0"], plain["held"])   # rake costs no launch and no byte
    dev.close()


@pytest.mark.timeout(60)
def test_refused_rakes_leave_the_output_and_the_table_alone():
    s = case("turn_imperfect_recall")
    dev = device_of(s)
    lib = L.load()
    ids = action_ids(s["nodes"])
    b = np.ascontiguousarray(dev.board0, dtype=np.uint8)
    h = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in dev.h]
    keep = [np.ascontiguousarray(dev.cids[r][p], dtype=np.uint32) for r in range(len(dev.cids)) for p in (0, 1)]
    arr = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    game_args = (dev.table._h, dev.tree._h, vp(b), len(b), vp(h[0]), len(h[0]), vp(h[1]), len(h[1]), arr, len(dev.cids))
    n = np.asarray(ids, dtype=np.int32)
    total = int(lib.rs_node_report_size(dev.tree._h, len(b), len(h[0]), vp(n), len(n), None))
    out2, out_rep = np.full(2, 7.0), np.full(total, 7.0)
    params = L.RangeCfrParams()
    params.mode, params.sorted = 0, L.FORM_ON
    before = dev.download()

    def calls(rake):
        st, _alive = rk.arg(rake)
        handle = C.c_void_p()
        rc = (lib.rs_best_response_raked(*game_args, None, None, st, L.BR_MAX | L.BR_SORTED, out2.ctypes.data_as(C.POINTER(C.c_double))),
              lib.rs_node_report_raked(*game_args, None, None, st, L.BR_AVERAGE | L.BR_SORTED, 0, vp(n), len(n), vp(out_rep), len(out_rep)),
              lib.rs_range_cfr_create_raked(*game_args, None, None, st, C.byref(params), C.byref(handle)))
        return rc, handle

    refused = {"a negative rate": (-0.01, 30.0), "a rate above 1": (1.5, 30.0), "a NaN rate": (np.nan, 30.0), "an infinite rate": (np.inf, 30.0), "a NaN cap": (0.05, np.nan),
               "a negative cap": (0.05, -1.0), "reserved[0]": (0.05, 30.0, (1, 0)), "reserved[1]": (0.05, 30.0, (0, 7))}
    for what, rake in refused.items():
        rc, handle = calls(rake)
        assert rc == (L.ERR_INVALID,) * 3, (what, rc)
        assert b"rs_rake" in lib.rs_last_error(), (what, lib.rs_last_error())
        assert handle.value is None, what
        assert (out2 == 7.0).all() and (out_rep == 7.0).all(), what
        with pytest.raises(rs.RsError):
            br(dev, L.BR_MAX, rake)
    assert same_tables(dev.download(), before)
    rc, handle = calls((0.05, np.inf))                                              # uncapped: taken
    assert rc == (L.OK,) * 3 and handle.value is not None
    assert not (out2 == 7.0).any() and not (out_rep == 7.0).any()
    alt = np.zeros(len(h[1]))
    assert lib.rs_range_cfr_set_gadget(handle, 0, vp(alt)) == L.ERR_UNSUPPORTED     # the gadget is a zero-sum construction
    assert same_tables(dev.download(), before)
    lib.rs_range_cfr_destroy(handle)
    sv = solver(dev, RAKE)
    with pytest.raises(rs.RsError) as e:
        sv.set_gadget(0, alt)
    assert e.value.code == L.ERR_UNSUPPORTED
    sv.destroy()
    for rake in ((0.0, 30.0), (0.05, 0.0)):                                         # no rake: the gadget is welcome
        sv = solver(dev, rake)
        sv.set_gadget(0, alt)
        sv.destroy()
    assert same_tables(dev.download(), before)
    dev.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("algo,bound", [("cfr", 0.0191), ("rmplus", 0.0175)])
def test_200_iterations_solve_the_raked_game(algo, bound):
    """The 25 x 20 river game of test_gpu_range_cfr.test_200_iterations_solve_the_river_game under rake (0.05, 30), from zero tables.  The exploitability is
    rake.exploitability of two best_response_rounds calls (RS_BR_MAX and RS_BR_AVERAGE, both RS_BR_SORTED): the game is general-sum.  On the zero tables it is 76.728524
    chips per deal and the rake paid 5.050000.  tests/np_rake.py (train, 200 iterations, then its own exploitability) reaches 0.812711 with CFR (1.0592 % of the start,
    rake paid 2.617019) and 0.743581 with RM+ (0.9691 %, rake paid 2.620915); the bounds are 1.8 x those shares, the margin test_200_iterations_solve_the_river_game
    and the locks test give over their restatements, for a trajectory that differs from the restatement's by rounding."""
    board0, h, cids, sizes, tree = make_case("river_lanes")
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    dev = Device(board0, h, cids, sizes, tree)

    def measured():
        mx, avg = br(dev, L.BR_MAX | L.BR_SORTED, RAKE), br(dev, L.BR_AVERAGE | L.BR_SORTED, RAKE)
        return rk.exploitability(mx, avg), rk.paid(avg)

    zero, paid0 = measured()
    sig = {i: nbr.final_strategy(x) for i, x in nrc.zero_tables(nodes, sizes)[1].items()}
    want, want_paid = nr.exploitability(nodes, sig.__getitem__, game, cids, RAKE)
    close(zero, want, "the zero tables")
    close(paid0, want_paid, "the rake paid on the zero tables")
    assert abs(zero - 76.7285) < 1e-3 and abs(paid0 - 5.05) < 1e-3
    sv = solver(dev, RAKE, algo == "rmplus")
    values = sv.train(200)
    trained, paid = measured()
    print(algo, "exploitability of the raked game", zero, "->", trained, "share", trained / zero, "rake paid", paid0, "->", paid)
    assert trained < bound * zero, (algo, trained, zero)
    assert np.isfinite(values).all()
    assert paid < paid0                                                             # thin calls go first
    close(-(values[0] + values[1]), rk.paid(values), "paid")
    sv.destroy()
    dev.close()
