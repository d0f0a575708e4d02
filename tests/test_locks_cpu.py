"""CPU: the numpy restatement of node locks (tests/np_locks.py) against the identities their definition implies, on the cases tests/test_gpu_locks.py holds the device to.

  * a lock that factors through the card abstraction is a table edit: under locks.from_clusters(final_strategy(S'), cluster table) the locked walks agree with the unlocked
    oracle/np_br.py, tests/np_node_report.py and tests/np_range_cfr.py on the table whose node rows are S' -- the OTHER player's "max" value, both "avg" values, every
    node-report row and the cells a sweep writes at every OTHER node;
  * with every node of both players locked to the table's strategy "max" has nothing left to maximise: it equals the unlocked "avg";
  * the second summation order (reverse=) agrees, under locks that do NOT factor through the abstraction;
  * rs_node_lock_size against A * n_prefix * n_hands in all three rounds of a flop start, its refusals and the refusals of a bad lock that need no device.
f64 rows within RTOL, ATOL of test_np_br_cpu ("two summation orders of the same f64 sums"), table cells under test_range_cfr_cpu.compare_cells.
"""
import ctypes as C

import numpy as np
import pytest

import np_locks as nl
import np_node_report as nnr
import np_range_cfr as nrc
from oracle import np_br as nbr
from oracle import np_restate as npr
from test_node_report_cpu import close, rows_of, setup
from test_range_cfr_cpu import compare_cells, copy_of

CASES = ["river_wave_35", "turn_imperfect_recall", "flop_three_rounds"]


def from_clusters(sigma, table):
    from rustsolver_amd import locks
    return locks.from_clusters(sigma, table)


def pick_nodes(nodes):
    """the first action node, in tree order, of every (round, player) the tree has -> [tree node id]"""
    seen = {}
    for i, nd in enumerate(nodes):
        if nd["kind"] == "action":
            seen.setdefault((nd["round_idx"], nd["player"]), i)
    return [seen[k] for k in sorted(seen)]


def lock_shape(nodes, game, i):
    nd = nodes[i]
    return len(nd["children"]), len(game.ro) // game.per_prefix[nd["round_idx"]], game.n[nd["player"]]


def shares_a_card(nodes, game, board0, i):
    """bool [F][H]: the hand holds one of the prefix's new cards (no deal under that prefix: the lock's entries there are never used)"""
    nd = nodes[i]
    r, pp, n0 = nd["round_idx"], game.per_prefix[nd["round_idx"]], len(board0)
    new = game.ro[::pp, n0:n0 + r]                                                  # [F][r]
    return (game.hands[nd["player"]][None, :, :, None] == new[:, None, None, :]).any(axis=(2, 3))


def random_lock(rng, nodes, game, board0, i, garbage=False):
    """a strategy drawn afresh for every (prefix, hand): it differs inside every cluster and between prefixes -- no table row can say it.  garbage: finite nonsense (not
    a strategy) on the pairs that share a card"""
    A, F, H = lock_shape(nodes, game, i)
    x = rng.random((A, F, H)) + 0.05
    x[rng.random((A, F, H)) < 0.2] = 0.0                                            # pure and mixed columns
    x[0] += (x.sum(axis=0) == 0)
    lock = x / x.sum(axis=0)[None]
    if garbage:
        bad = shares_a_card(nodes, game, board0, i)
        lock = np.where(bad[None], rng.random((A, F, H)) * 1e3, lock)
    return np.ascontiguousarray(lock)


def random_locks(name, garbage=False, seed=5):
    s = setup(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    return {i: random_lock(rng, s["nodes"], s["game"], s["board0"], i, garbage) for i in pick_nodes(s["nodes"])}


def row_like(rng, shape):
    """a strategy-sum row of random_tables' kind: uniform [0, 10) with 15 % zeros"""
    return np.where(rng.random(shape) < 0.15, 0.0, rng.random(shape) * 10.0).astype(np.float32)


@pytest.mark.parametrize("name", CASES)
def test_a_lock_that_factors_through_the_abstraction_is_a_table_edit(name):
    s = setup(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    picked = pick_nodes(nodes)
    assert len(picked) == 2 * len(cids)                                             # a node of each player in every round the case has
    rng = np.random.Generator(np.random.PCG64(71))
    for i in picked:
        nd = nodes[i]
        idx, P, r = nd["index"], nd["player"], nd["round_idx"]
        R, S = copy_of(*s["tables"])
        Rp, Sp = copy_of(R, S)
        Rp[idx] = Sp[idx] = row_like(rng, S[idx].shape)                            # the edited table: get_strategy and get_final_strategy are one text, so one row
        sig_row = nbr.final_strategy(Sp[idx])                                       # serves the readers of the sums and the sweep, which reads the regrets
        assert sig_row.tobytes() == npr.get_strategy_f32(Rp[idx]).tobytes()
        locks = {i: from_clusters(sig_row, cids[r][P])}
        assert locks[i].shape == lock_shape(nodes, game, i)
        sig, sig_p = nnr.strategies((R, S)), nnr.strategies((Rp, Sp))
        what = (name, i)
        got = nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks)
        want = nbr.best_response(nodes, sig_p.__getitem__, None, None, cids, "max", None, game)
        close(got[1 - P], want[1 - P], what + ("max, the other player",))
        assert got[P] <= want[P] + 1e-9                                             # the locked player no longer maximises at the node
        close(nl.best_response(nodes, sig.__getitem__, game, cids, "avg", locks),
              nbr.best_response(nodes, sig_p.__getitem__, None, None, cids, "avg", None, game), what + ("avg",))
        for p in (0, 1):
            got, want = nl.report(nodes, sig.__getitem__, game, cids, p, locks), nnr.report(nodes, sig_p.__getitem__, game, cids, p)
            assert sorted(got) == sorted(want)
            for k in want:
                for (row, x), (_, y) in zip(rows_of(got[k]), rows_of(want[k])):
                    close(x, y, what + (p, k, row))
            A, B = copy_of(R, S), copy_of(Rp, Sp)
            va, vb = nl.sweep(nodes, A[0], A[1], game, cids, p, False, locks), nrc.sweep(nodes, B[0], B[1], game, cids, p)
            close(va, vb, what + (p, "sweep value"))
            assert A[0][idx].tobytes() == R[idx].tobytes() and A[1][idx].tobytes() == S[idx].tobytes()   # the locked node's rows: neither read nor written
            moved = 0
            for k in R:
                if k == idx:
                    continue
                for t in (0, 1):
                    compare_cells(A[t][k], B[t][k], what + (p, k, t))
                    moved += A[t][k].tobytes() != (R, S)[t][k].tobytes()
            assert moved > 0


@pytest.mark.parametrize("name", CASES)
def test_with_every_node_locked_to_the_tables_strategy_max_is_avg(name):
    s = setup(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    sig = nnr.strategies(s["tables"])
    locks = {i: from_clusters(sig[nd["index"]], cids[nd["round_idx"]][nd["player"]]) for i, nd in enumerate(nodes) if nd["kind"] == "action"}
    want = nbr.best_response(nodes, sig.__getitem__, None, None, cids, "avg", None, game)
    close(nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks), want, (name, "max under locks"))
    close(nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks, real=True), want, (name, "max in the real game under locks"))
    free = nbr.best_response(nodes, sig.__getitem__, None, None, cids, "max", None, game)
    assert (free > want + 1e-6).all()                                               # which the free responder beats


@pytest.mark.parametrize("name", CASES)
def test_the_reversed_summation_order_agrees(name):
    """locks that do not factor through the abstraction, garbage on the pairs that share a card where the case has such pairs"""
    s = setup(name)
    nodes, game, cids = s["nodes"], s["game"], s["cids"]
    locks = random_locks(name, garbage=len(s["board0"]) < 5)
    if len(s["board0"]) < 5:
        assert any(shares_a_card(nodes, game, s["board0"], i).any() for i in locks)
    for current in (False, True):
        sig = nnr.strategies(s["tables"], current)
        for mode in ("max", "avg"):
            close(nl.best_response(nodes, sig.__getitem__, game, cids, mode, locks), nl.best_response(nodes, sig.__getitem__, game, cids, mode, locks, reverse=True), (name, mode))
        close(nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks, real=True),
              nl.best_response(nodes, sig.__getitem__, game, cids, "max", locks, real=True, reverse=True), (name, "real"))
    sig = nnr.strategies(s["tables"])
    for p in (0, 1):
        fwd, rev = nl.report(nodes, sig.__getitem__, game, cids, p, locks), nl.report(nodes, sig.__getitem__, game, cids, p, locks, reverse=True)
        for k in fwd:
            for (row, x), (_, y) in zip(rows_of(fwd[k]), rows_of(rev[k])):
                close(x, y, (name, p, k, row))
        for rmplus in (False, True):
            A, B = copy_of(*s["tables"]), copy_of(*s["tables"])
            close(nl.sweep(nodes, A[0], A[1], game, cids, p, rmplus, locks), nl.sweep(nodes, B[0], B[1], game, cids, p, rmplus, locks, reverse=True), (name, p, rmplus))
            for k in A[0]:
                for t in (0, 1):
                    compare_cells(A[t][k], B[t][k], (name, p, rmplus, k, t))


def test_the_wrappers_helpers_shape_and_cut_locks():
    """locks.from_clusters, locks.pure and locks.drop_columns: pure numpy on the host tree"""
    import rustsolver_amd as rs
    from rustsolver_amd import locks as lk

    t = setup("turn_imperfect_recall")
    nodes, game, cids = t["nodes"], t["game"], t["cids"]
    _, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=t["tree"][0], raise_sizes=t["tree"][1]))
    sig = nnr.strategies(t["tables"])
    for i in pick_nodes(nodes):
        nd = nodes[i]
        A, F, H = lock_shape(nodes, game, i)
        lock = lk.from_clusters(sig[nd["index"]], cids[nd["round_idx"]][nd["player"]])
        assert lock.shape == (A, F, H) and lock.dtype == np.float64
        for f in (0, F - 1):
            for h in (0, H - 1):
                assert lock[:, f, h].tolist() == sig[nd["index"]][:, int(cids[nd["round_idx"]][nd["player"]][f, h])].astype(np.float64).tolist()
        one = lk.pure(tree, i, 1, F, H)
        assert one.shape == (A, F, H) and one.sum() == F * H and (one[1] == 1.0).all()
        keep = [np.ones(game.n[0], dtype=bool), np.ones(game.n[1], dtype=bool)]
        keep[nd["player"]][[0, 2]] = False
        cut = lk.drop_columns(tree, {i: lock}, keep)
        assert cut[i].tobytes() == np.ascontiguousarray(lock[:, :, keep[nd["player"]]]).tobytes()
        assert lk.drop_columns(tree, {i: lock}, [None, None])[i] is not None and lk.drop_columns(tree, None, keep) is None
    with pytest.raises(ValueError):
        lk.pure(tree, pick_nodes(nodes)[0], 9, 1, 3)
    with pytest.raises(ValueError):
        lk.from_clusters(np.zeros(3), np.zeros((1, 3)))


def test_lock_size_and_the_refusals_that_need_no_device():
    """rs_node_lock_size = A * n_prefix * n_hands in the three rounds of a flop start; bad arguments give 0; a bad lock is refused before anything else is looked at"""
    import rustsolver_amd as rs
    from rustsolver_amd import _lib as L
    from rustsolver_amd import locks as lk

    s = setup("flop_three_rounds")
    nodes, game, board0 = s["nodes"], s["game"], s["board0"]
    lib = L.load()
    _, tree = rs.build_game_tree(rs.Options(n_board_cards=3, bet_sizes=s["tree"][0], raise_sizes=s["tree"][1]))
    picked = pick_nodes(nodes)
    assert sorted(nodes[i]["round_idx"] for i in picked) == [0, 0, 1, 1, 2, 2]
    for i in picked:
        A, F, H = lock_shape(nodes, game, i)
        assert F == (1, 49, 49 * 48)[nodes[i]["round_idx"]]
        assert lib.rs_node_lock_size(tree._h, 3, H, i) == A * F * H
        assert lk.pure(tree, i, A - 1, F, H).shape == (A, F, H) and lk.pure(tree, i, A - 1, F, H)[A - 1].min() == 1.0
    terminal = next(i for i, nd in enumerate(nodes) if nd["kind"] == "terminal")
    first = picked[0]
    for args in ((3, 6, 0), (3, 6, terminal), (3, 6, len(nodes)), (3, 6, -1), (2, 6, first), (6, 6, first), (3, 0, first), (3, 1327, first)):
        assert lib.rs_node_lock_size(tree._h, *args) == 0, args
        assert lib.rs_last_error().startswith(b"rs_node_locks"), args
    assert lib.rs_node_lock_size(None, 3, 6, first) == 0
    # turn-start tree: a node of the second round has 48 prefixes, none of a third round exists
    t = setup("turn_imperfect_recall")
    _, turn_tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=t["tree"][0], raise_sizes=t["tree"][1]))
    for i in pick_nodes(t["nodes"]):
        A, F, H = lock_shape(t["nodes"], t["game"], i)
        assert lib.rs_node_lock_size(turn_tree._h, 4, H, i) == A * F * H
        assert lib.rs_node_lock_size(turn_tree._h, 5, H, i) == (A * H if t["nodes"][i]["round_idx"] == 0 else 0)
    # a bad lock is refused by rs_best_response_locked before the table (NULL here) is looked at; `out` stays
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    b = np.ascontiguousarray(t["board0"], dtype=np.uint8)
    h = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in t["h"]]
    out = np.full(2, 7.0)
    node = pick_nodes(t["nodes"])[-1]
    good = random_lock(np.random.Generator(np.random.PCG64(3)), t["nodes"], t["game"], t["board0"], node, garbage=True)

    def call(ids, rows):
        ids = np.asarray(ids, dtype=np.int32)
        ptrs = (C.c_void_p * max(len(rows), 1))(*[None if r is None else r.ctypes.data for r in rows])
        st = L.NodeLocks()
        st.n, st.nodes, st.sigma = len(ids), ids.ctypes.data, C.cast(ptrs, C.c_void_p).value
        return lib.rs_best_response_locked(None, turn_tree._h, vp(b), 4, vp(h[0]), len(h[0]), vp(h[1]), len(h[1]), None, 2, None, C.byref(st), L.BR_MAX,
                                           out.ctypes.data_as(C.POINTER(C.c_double)))

    def spoiled(value, pair_shares):
        bad = shares_a_card(t["nodes"], t["game"], t["board0"], node)
        f, hh = [int(x[0]) for x in np.nonzero(bad if pair_shares else ~bad)]
        x = good.copy()
        x[1, f, hh] = value
        return x

    refused = {"a terminal node": ([terminal], [good]), "an id out of range": ([len(t["nodes"])], [good]), "a negative id": ([-1], [good]),
               "an id twice": ([node, node], [good, good]), "a NULL row": ([node], [None]),
               "a NaN": ([node], [spoiled(np.nan, False)]), "an infinity": ([node], [spoiled(np.inf, False)]), "a negative entry": ([node], [spoiled(-0.25, False)]),
               "a NaN on a pair that shares a card": ([node], [spoiled(np.nan, True)]), "a negative entry on a pair that shares a card": ([node], [spoiled(-1.0, True)]),
               "a column that sums to 1 + 1e-8": ([node], [spoiled(good[1][~shares_a_card(t["nodes"], t["game"], t["board0"], node)][0] + 1e-8, False)])}
    for what, (ids, rows) in refused.items():
        assert call(ids, rows) == L.ERR_INVALID, what
        assert b"rs_node_locks" in lib.rs_last_error(), (what, lib.rs_last_error())
        assert (out == 7.0).all(), what
    assert call([node], [good]) == L.ERR_INVALID and b"rs_best_response: NULL argument" in lib.rs_last_error()   # the lock itself passes: the NULL table is what is wrong
    assert call([node], [spoiled(good[1][~shares_a_card(t["nodes"], t["game"], t["board0"], node)][0] + 1e-10, False)]) == L.ERR_INVALID and b"NULL argument" in lib.rs_last_error()
    assert (out == 7.0).all()
