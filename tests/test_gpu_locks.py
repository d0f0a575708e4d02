"""GPU (-m gpu): node locks (rs_best_response_locked, rs_node_report_locked, rs_range_cfr_create_locked) against the numpy restatement tests/np_locks.py.

The cases are the small ones of tests/test_locks_cpu.py, chosen for the two lock kernels' indexing (a thread per lane, lock row = (run-out / run-outs per prefix, hand)):
river games of 70 / 66 hands (a 256-thread block ends inside a row), a turn game of 48 run-outs times 9 / 7 hands (blocks straddle prefixes), a flop start of 6 x 5 hands
where 2 352 / 48 / 1 run-outs per prefix meet in one call, and the 8-action tree of tests/test_gpu_range_cfr_edges.py with its widest node locked (the kernels' unrolled
action predicate up to RS_MAX_ACTIONS).  The locks are drawn per (prefix, hand): no table row can express them.  f64 rows within RTOL, ATOL of test_np_br_cpu, table
cells as test_gpu_range_cfr.compare_sweep compares them; tests/test_locks_cpu.py holds the restatement's own two summation orders to the same numbers.
"""
import ctypes as C

import numpy as np
import pytest

import np_locks as nl
import np_node_report as nnr
import np_range_cfr as nrc
import np_weighted as nw
import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from test_gpu_br_pinned import depth_first
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, make_case, same_tables
from test_locks_cpu import lock_shape, pick_nodes, random_lock, shares_a_card
from test_node_report_cpu import close, rows_of, setup
from test_range_cfr_cpu import first_node_of, make_shape, random_tables

pytestmark = pytest.mark.gpu

CASES = ["river_wave_35", "turn_imperfect_recall", "flop_three_rounds", "river_eight_actions_thread"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


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


def locked_nodes(nodes):
    """a node of each player in every round, and each player's first node of RS_MAX_ACTIONS actions where the tree has one"""
    picked = pick_nodes(nodes)
    for p in (0, 1):
        wide = [i for i, nd in enumerate(nodes) if nd["kind"] == "action" and nd["player"] == p and len(nd["children"]) == L.MAX_ACTIONS]
        picked += [i for i in wide[:1] if i not in picked]
    return picked


_LOCKS = {}


def locks_of(name):
    """seeded random strategies per (prefix, hand); garbage-but-finite entries on the pairs that share a card where the game has such pairs"""
    if name not in _LOCKS:
        s = case(name)
        rng = np.random.Generator(np.random.PCG64(5))
        _LOCKS[name] = {i: random_lock(rng, s["nodes"], s["game"], s["board0"], i, garbage=len(s["board0"]) < 5) for i in locked_nodes(s["nodes"])}
    return _LOCKS[name]


def device_of(name):
    s = case(name)
    dev = Device(s["board0"], s["h"], s["cids"], s["sizes"], s["tree"])
    assert dev.tree.n_nodes == len(s["nodes"])
    for nd, want in zip(dev.tree.nodes, s["nodes"]):
        assert (nd.kind == L.NODE_ACTION) == (want["kind"] == "action") and (nd.kind != L.NODE_ACTION or nd.index == want["index"])
    dev.upload(*s["tables"])
    return s, dev


def br(dev, mode, locks, **kw):
    return dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, mode, locks=locks, **kw)


def report(dev, p, ids, locks, **kw):
    return dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, locks=locks, **kw)


def solver(dev, locks, rmplus=False, sorted_showdowns=True):
    return rs.RangeCFR(dev.table, dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns, locks=locks)


def action_ids(nodes):
    return [i for i, nd in enumerate(nodes) if nd["kind"] == "action"]


def same_reports(a, b):
    return sorted(a) == sorted(b) and all(x.tobytes() == y.tobytes() for i in a for (_, x), (_, y) in zip(rows_of(a[i]), rows_of(b[i])))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", CASES + ["turn_slices_7_8"])
def test_locks_that_no_table_can_express_equal_the_restatement(name):
    """best response in every mode, every node-report row and one full-width sweep per traverser.  Without the feature nothing here can pass: the wrappers have no locks=
    and no table row plays a strategy that differs inside a cluster"""
    s, dev = device_of(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    locks = locks_of(name)
    if name == "river_eight_actions_thread":
        assert max(lock.shape[0] for lock in locks.values()) == L.MAX_ACTIONS
    if len(s["board0"]) < 5:
        assert any(shares_a_card(nodes, game, s["board0"], i).any() for i in locks)
    for current in (False, True):
        sig = nnr.strategies(s["tables"], current)
        want = {L.BR_MAX: nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks),
                L.BR_AVERAGE: nl.best_response(nodes, sig.__getitem__, game, cids, "avg", locks),
                L.BR_MAX | L.BR_REAL: nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks, real=True)}
        free = nbr.best_response(nodes, sig.__getitem__, None, None, cids, "avg", None, game)
        assert not np.allclose(want[L.BR_AVERAGE], free, rtol=1e-6, atol=1e-9)      # the locks matter
        for mode, w in want.items():
            for sorted_bit in (L.BR_SORTED, 0):
                got = br(dev, mode | sorted_bit, locks, current=current)
                print(name, "mode", hex(mode | sorted_bit), "current", current, got, w)
                close(got, w, (name, mode, sorted_bit, current))
        ids = action_ids(nodes)
        for p in (0, 1):
            w = nl.report(nodes, sig.__getitem__, game, cids, p, locks)
            for sorted_showdowns in ((True, False) if not current else (True,)):
                got = report(dev, p, ids, locks, current=current, sorted_showdowns=sorted_showdowns)
                assert sorted(got) == sorted(w)
                for i in w:
                    for (row, x), (_, y) in zip(rows_of(got[i]), rows_of(w[i])):
                        close(x, y, (name, p, current, sorted_showdowns, i, row))
    cells = differ = 0
    for p in (0, 1):
        before = copy_tables(*s["tables"])
        want = copy_tables(*before)
        value = nl.sweep(nodes, want[0], want[1], game, cids, p, bool(p), locks)     # plain for traverser 0, RM+ for traverser 1
        for sorted_showdowns in (True, False):
            dev.upload(*before)
            sv = solver(dev, locks, bool(p), sorted_showdowns)
            got_value = sv.iterate(p)
            got = dev.download()
            sv.destroy()
            close(got_value, value, (name, p, sorted_showdowns, "sweep value"))
            c, d, _ = compare_sweep(nodes, game, cids, p, before, got, want, (name, p, sorted_showdowns))
            cells, differ = cells + c, differ + d
            for i in locks:
                idx = nodes[i]["index"]
                assert got[0][idx].tobytes() == before[0][idx].tobytes() and got[1][idx].tobytes() == before[1][idx].tobytes(), (name, p, i)
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    dev.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["river_wave_35", "turn_imperfect_recall", "flop_three_rounds", "turn_slices_7_8"])
def test_both_tree_orders_repeats_and_lock_order_give_the_same_bits(name):
    s, dev = device_of(name)
    nodes = s["nodes"]
    ids = action_ids(nodes)
    full = locks_of(name)
    flipped = {i: full[i] for i in reversed(list(full))}
    part = {i: full[i] for i in list(full)[::2]}
    part_flipped = {i: part[i] for i in reversed(list(part))}
    modes = (L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE, L.BR_MAX | L.BR_REAL | L.BR_SORTED)

    def everything(locks):
        out = dict(br=[br(dev, m, locks) for m in modes], rep=[report(dev, p, ids, locks) for p in (0, 1)])
        dev.upload(*s["tables"])
        sv = solver(dev, locks)
        out["values"] = [sv.iterate(0), sv.iterate(1)]
        out["launches"] = sv.launches()
        out["tables"] = dev.download()
        sv.destroy()
        dev.upload(*s["tables"])
        return out

    def same(a, b):
        return (all(x.tobytes() == y.tobytes() for x, y in zip(a["br"], b["br"])) and all(same_reports(x, y) for x, y in zip(a["rep"], b["rep"]))
                and a["values"] == b["values"] and same_tables(a["tables"], b["tables"]))

    levels = everything(full)
    assert levels["launches"] > 0
    assert same(everything(full), levels), (name, "twice")
    assert same(everything(flipped), levels), (name, "the locks in another order")
    with depth_first():
        walk = everything(full)
        assert walk["launches"] == -1
        walk_part = everything(part_flipped)
    assert same(walk, levels), (name, "depth first")
    some = everything(part)
    assert same(walk_part, some), (name, "a subset in another order, depth first")
    assert not same(some, levels)                                                   # fewer locks: another game
    dev.close()


@pytest.mark.timeout(60)
def test_the_table_is_untouched_at_a_locked_node():
    """three iterations without ticks: the locked nodes' regret and strategy-sum rows keep their uploaded bytes, every other node's rows have moved"""
    name = "turn_imperfect_recall"
    s, dev = device_of(name)
    locks = locks_of(name)
    before = dev.download()
    assert same_tables(before, s["tables"])
    for rmplus in (False, True):
        dev.upload(*s["tables"])
        sv = solver(dev, locks, rmplus)
        sv.train(3)
        after = dev.download()
        sv.destroy()
        locked = {s["nodes"][i]["index"] for i in locks}
        for idx in before[0]:
            kept = after[0][idx].tobytes() == before[0][idx].tobytes(), after[1][idx].tobytes() == before[1][idx].tobytes()
            assert kept == ((True, True) if idx in locked else (False, False)), (rmplus, idx, kept)
    dev.close()


@pytest.mark.timeout(60)
def test_without_locks_the_existing_entry_points_answer():
    """locks=None and locks={}: the bytes of rs_best_response_weighted and rs_node_report_weighted, and of a solver of rs_range_cfr_create_weighted its values, tables,
    launches and held bytes"""
    name = "turn_imperfect_recall"
    s, dev = device_of(name)
    lib = L.load()
    ids = action_ids(s["nodes"])
    b = np.ascontiguousarray(dev.board0, dtype=np.uint8)
    h = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in dev.h]
    keep = [np.ascontiguousarray(dev.cids[r][p], dtype=np.uint32) for r in range(len(dev.cids)) for p in (0, 1)]
    arr = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    game = (dev.table._h, dev.tree._h, vp(b), len(b), vp(h[0]), len(h[0]), vp(h[1]), len(h[1]), arr, len(dev.cids))
    for mode in (L.BR_MAX, L.BR_AVERAGE | L.BR_SORTED, L.BR_MAX | L.BR_REAL | L.BR_SORTED | L.BR_CURRENT):
        out = np.zeros(2)
        L.check(lib.rs_best_response_weighted(*game, None, mode, out.ctypes.data_as(C.POINTER(C.c_double))))
        for locks in (None, {}):
            assert br(dev, mode, locks).tobytes() == out.tobytes(), (mode, locks)
    n = np.asarray(ids, dtype=np.int32)
    for p in (0, 1):
        total = int(lib.rs_node_report_size(dev.tree._h, len(b), len(h[p]), vp(n), len(n), None))
        out = np.zeros(total)
        L.check(lib.rs_node_report_weighted(*game, None, L.BR_AVERAGE | L.BR_SORTED, p, vp(n), len(n), vp(out), len(out)))
        for locks in (None, {}):
            got = report(dev, p, ids, locks)
            assert np.concatenate([x.reshape(-1) for i in ids for _, x in rows_of(got[i])]).tobytes() == out.tobytes(), (p, locks)
    handle = C.c_void_p()
    params = L.RangeCfrParams()
    params.mode, params.sorted = 0, L.FORM_ON
    L.check(lib.rs_range_cfr_create_weighted(*game, None, C.byref(params), C.byref(handle)))
    held0 = int(lib.rs_range_cfr_bytes(handle))
    values = []
    for p in (0, 1):
        v = C.c_double(0.0)
        L.check(lib.rs_range_cfr_iterate(handle, p, C.byref(v)))
        values.append(v.value)
    plain = dict(values=values, launches=int(lib.rs_range_cfr_launches(handle)), held=int(lib.rs_range_cfr_bytes(handle)), tables=dev.download())
    lib.rs_range_cfr_destroy(handle)
    for locks in (None, {}):
        dev.upload(*s["tables"])
        sv = solver(dev, locks)
        assert sv.nbytes == held0
        assert [sv.iterate(0), sv.iterate(1)] == plain["values"]
        assert sv.launches() == plain["launches"] and sv.nbytes == plain["held"]
        assert same_tables(dev.download(), plain["tables"])
        sv.destroy()
    dev.upload(*s["tables"])
    sv = solver(dev, locks_of(name))                                                # the locks' rows are the object's: counted
    assert sv.nbytes > held0
    sv.destroy()
    dev.close()


@pytest.mark.timeout(60)
def test_hands_of_weight_zero_take_their_lock_columns_with_them():
    """weights= with zeros and the locks given over the full ranges: the bytes of the call on the shortened ranges with the locks' columns cut by hand"""
    name = "turn_imperfect_recall"
    s, dev = device_of(name)
    nodes = s["nodes"]
    locks = locks_of(name)
    rng = np.random.Generator(np.random.PCG64(17))
    w = [rng.random(len(h)) + 0.5 for h in dev.h]
    w[0][[1, 4]] = 0.0
    w[1][[0, 6]] = 0.0
    keep = [x != 0.0 for x in w]
    h = [np.asarray(dev.h[p])[keep[p]] for p in (0, 1)]
    cids = [[np.asarray(row[p])[:, keep[p]] for p in (0, 1)] for row in dev.cids]
    cut = {i: np.ascontiguousarray(lock[:, :, keep[nodes[i]["player"]]]) for i, lock in locks.items()}
    wk = [w[p][keep[p]] for p in (0, 1)]
    ids = action_ids(nodes)
    for deal in ("sequential", "joint"):
        for mode in (L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE):
            got = dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, mode, weights=w, deal=deal, locks=locks)
            want = dev.table.best_response_rounds(dev.tree, dev.board0, h[0], h[1], cids, mode, weights=wk, deal=deal, locks=cut)
            assert got.tobytes() == want.tobytes(), (deal, mode)
            assert got.tobytes() != dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, mode, weights=w, deal=deal).tobytes()
        for p in (0, 1):
            got = dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, weights=w, deal=deal, locks=locks)
            want = dev.table.node_report(dev.tree, dev.board0, h[0], h[1], cids, p, ids, weights=wk, deal=deal, locks=cut)
            for i in ids:
                for (row, x), (_, y) in zip(rows_of(got[i]), rows_of(want[i])):
                    assert x[..., keep[p]].tobytes() == y.tobytes() and not x[..., ~keep[p]].any(), (deal, p, i, row)
        values = []
        for args in ((dev.h, dev.cids, w, locks), (h, cids, wk, cut)):
            dev.upload(*s["tables"])
            sv = rs.RangeCFR(dev.table, dev.tree, dev.board0, args[0][0], args[0][1], args[1], weights=args[2], deal=deal, locks=args[3])
            values.append(([sv.iterate(0), sv.iterate(1)], dev.download()))
            sv.destroy()
        assert values[0][0] == values[1][0] and same_tables(values[0][1], values[1][1]), deal
    dev.upload(*s["tables"])
    game = nw.WeightedGame(dev.board0, h, wk, "joint")                              # and the restatement on a WeightedGame
    sig = nnr.strategies(s["tables"])
    got = dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, L.BR_MAX | L.BR_SORTED, weights=w, deal="joint", locks=locks)
    close(got, nl.best_response(nodes, sig.__getitem__, game, cids, "max", cut), "weighted, joint")
    dev.close()


def solve_game():
    """the 25 x 20 river game of test_gpu_range_cfr.test_200_iterations_solve_the_river_game with player 1's first node locked to a seeded random per-hand strategy"""
    board0, h, cids, sizes, tree = make_case("river_lanes")
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    node = nodes.index(first_node_of(nodes, 1))
    locks = {node: random_lock(np.random.Generator(np.random.PCG64(9)), nodes, game, board0, node)}
    return nodes, game, cids, sizes, locks, board0, h, tree


@pytest.mark.timeout(120)
@pytest.mark.parametrize("algo,bound", [("cfr", 0.0207), ("rmplus", 0.018)])
def test_200_iterations_solve_the_game_around_a_lock(algo, bound):
    """The exploitability INSIDE the locked game -- best_response_rounds(locks=) under RS_BR_MAX | RS_BR_SORTED, sum / 2: the locked node maximises nothing -- after 200
    iterations from zero tables against its value on the zero tables (70.77 chips per deal).  tests/np_locks.py (train, 200 iterations, then best_response "max" under
    the lock) reaches 1.153 % of it with CFR (0.816 chips) and 0.999 % with RM+ (0.707 chips); the bounds are 1.8 x those shares, the margin
    test_200_iterations_solve_the_river_game gives over its restatement, for a trajectory that differs from the restatement's by rounding."""
    nodes, game, cids, sizes, locks, board0, h, tree = solve_game()
    dev = Device(board0, h, cids, sizes, tree)
    expl = lambda: br(dev, L.BR_MAX | L.BR_SORTED, locks).sum() / 2.0
    zero = expl()
    sig = {i: nbr.final_strategy(x) for i, x in nrc.zero_tables(nodes, sizes)[1].items()}
    close(zero, nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks).sum() / 2.0, "the zero tables")
    sv = solver(dev, locks, algo == "rmplus")
    values = sv.train(200)
    trained = expl()
    print(algo, "exploitability inside the locked game", zero, "->", trained, "share", trained / zero)
    assert trained < bound * zero, (algo, trained, zero)
    assert np.isfinite(values).all()
    R, S = dev.download()
    idx = nodes[next(iter(locks))]["index"]
    assert not R[idx].any() and not S[idx].any()                                   # the locked node's rows were never written
    sv.destroy()
    dev.close()


@pytest.mark.timeout(60)
def test_refused_locks_leave_the_output_and_the_table_alone():
    name = "turn_imperfect_recall"
    s, dev = device_of(name)
    nodes, game, board0 = s["nodes"], s["game"], s["board0"]
    lib = L.load()
    ids = action_ids(nodes)
    terminal = next(i for i, nd in enumerate(nodes) if nd["kind"] == "terminal")
    chance = next(i for i, nd in enumerate(nodes) if nd["kind"] not in ("action", "terminal"))
    node = pick_nodes(nodes)[-1]                                                    # last round: 48 prefixes, pairs that share a card
    good = random_lock(np.random.Generator(np.random.PCG64(3)), nodes, game, board0, node, garbage=True)
    bad_pair = shares_a_card(nodes, game, board0, node)
    assert bad_pair.any() and not bad_pair.all()

    def spoiled(value, pair_shares):
        f, hh = [int(x[-1]) for x in np.nonzero(bad_pair if pair_shares else ~bad_pair)]
        x = good.copy()
        x[1, f, hh] = value
        return x

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

    def calls(lock_ids, rows):
        lock_ids = np.asarray(lock_ids, dtype=np.int32)
        ptrs = (C.c_void_p * max(len(rows), 1))(*[None if r is None else r.ctypes.data for r in rows])
        st = L.NodeLocks()
        st.n, st.nodes, st.sigma = len(lock_ids), lock_ids.ctypes.data, C.cast(ptrs, C.c_void_p).value
        handle = C.c_void_p()
        rc = (lib.rs_best_response_locked(*game_args, None, C.byref(st), L.BR_MAX | L.BR_SORTED, out2.ctypes.data_as(C.POINTER(C.c_double))),
              lib.rs_node_report_locked(*game_args, None, C.byref(st), L.BR_AVERAGE | L.BR_SORTED, 0, vp(n), len(n), vp(out_rep), len(out_rep)),
              lib.rs_range_cfr_create_locked(*game_args, None, C.byref(st), C.byref(params), C.byref(handle)))
        return rc, handle

    first_free = good[1][~bad_pair][-1]
    refused = {"a terminal node": ([terminal], [good]), "a chance node": ([chance], [good]), "an id out of range": ([len(nodes)], [good]), "a negative id": ([-1], [good]),
               "an id twice": ([node, node], [good, good]), "a NULL row": ([node], [None]),
               "a NaN": ([node], [spoiled(np.nan, False)]), "an infinity": ([node], [spoiled(np.inf, False)]), "a negative entry": ([node], [spoiled(-0.25, False)]),
               "a NaN on a pair that shares a card": ([node], [spoiled(np.nan, True)]), "a negative entry on a pair that shares a card": ([node], [spoiled(-1.0, True)]),
               "a column that sums to 1 + 1e-8": ([node], [spoiled(first_free + 1e-8, False)])}
    short = good.copy()
    short[0] *= 1.0 - 1e-7                                                          # every column that plays action 0 at all now sums to less than 1
    assert (np.abs(short.sum(axis=0) - 1.0)[~bad_pair] > 1e-9).any()
    refused["columns that sum to less than 1"] = ([node], [short])
    for what, (lock_ids, rows) in refused.items():
        rc, handle = calls(lock_ids, rows)
        assert rc == (L.ERR_INVALID,) * 3, (what, rc)
        assert b"rs_node_locks" in lib.rs_last_error(), (what, lib.rs_last_error())
        assert handle.value is None, what
        assert (out2 == 7.0).all() and (out_rep == 7.0).all(), what
    assert same_tables(dev.download(), before)
    rc, handle = calls([node], [spoiled(first_free + 1e-10, False)])                # within 1e-9 of 1: taken, and used as given
    assert rc == (L.OK,) * 3 and handle.value is not None
    assert not (out2 == 7.0).any() and not (out_rep == 7.0).any()
    alt = np.zeros(len(h[1]))
    assert lib.rs_range_cfr_set_gadget(handle, 0, vp(alt)) == L.ERR_UNSUPPORTED     # a gadget and locks on one object: out of scope
    assert same_tables(dev.download(), before)
    lib.rs_range_cfr_destroy(handle)
    with pytest.raises(rs.RsError):
        br(dev, L.BR_MAX, {terminal: good})
    with pytest.raises(ValueError):
        br(dev, L.BR_MAX, {node: good[:, :-1]})                                    # not [A][n_prefix][n_hands]
    sv = solver(dev, {node: good})
    with pytest.raises(rs.RsError) as e:
        sv.set_gadget(0, alt)
    assert e.value.code == L.ERR_UNSUPPORTED
    sv.destroy()
    assert same_tables(dev.download(), before)
    dev.close()
