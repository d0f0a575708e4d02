"""GPU (-m gpu): the node report (rs_node_report, rs_deal_trainer_node_report) against the numpy restatement tests/np_node_report.py.

Every row of every action node -- cfv[a], value, mass, own -- is compared with the restatement within RTOL, ATOL of test_np_br_cpu ("two summation orders of the same f64
sums"; tests/test_node_report_cpu.py holds the restatement's own two orders to the same numbers on the same cases).  The cases: river games of 70 and 66 hands (a 64-pair
workgroup ends inside a row, last-round form), a turn game of 48 run-outs and 9 / 7 hands (blocks straddle prefixes), a one-hand range and hands that meet no opponent
(mass 0, all-zero pairs), and a flop-start game of 6 x 5 hands where the fold lengths 2 352 / 48 / 1 meet in one call.  Then: the same bits from the level plan and the
depth-first walk, from a call repeated and from a subset of the nodes; no side effects on the table or on the calls that share its walk; i32 and binary16 tables and the
trainer's form on the trainers of test_gpu_br_pinned; refusals that leave the output buffer and the table alone."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import np_node_report as nnr
import rustsolver_amd as rs
from oracle import np_br as nbr
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from test_gpu_br_pinned import depth_first
from test_gpu_range_cfr import SLICES, Device, same_tables, trainer_game
from test_node_report_cpu import CASES, close, report_case, restated, rows_of, setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def device_of(name):
    """the case on the device with test_node_report_cpu.setup's tables uploaded; the tree's node ids are the restated tree's"""
    s = setup(name)
    dev = Device(s["board0"], s["h"], s["cids"], s["sizes"], s["tree"])
    assert dev.tree.n_nodes == len(s["nodes"])
    for nd, want in zip(dev.tree.nodes, s["nodes"]):
        assert (nd.kind == L.NODE_ACTION) == (want["kind"] == "action") and (nd.kind != L.NODE_ACTION or nd.index == want["index"])
    dev.upload(*s["tables"])
    return s, dev


def action_ids(nodes):
    return [i for i, nd in enumerate(nodes) if nd["kind"] == "action"]


def report(dev, p, ids, **kw):
    return dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, **kw)


def same_reports(a, b):
    return sorted(a) == sorted(b) and all(x.tobytes() == y.tobytes() for i in a for (_, x), (_, y) in zip(rows_of(a[i]), rows_of(b[i])))


def compare(got, want, what):
    assert sorted(got) == sorted(want), what
    for i in want:
        for (row, x), (_, y) in zip(rows_of(got[i]), rows_of(want[i])):
            assert x.dtype == np.float64
            close(x, y, (what, i, row))


@pytest.mark.parametrize("name", CASES + SLICES)
def test_report_equals_the_restatement(name):
    """every action node, both traversers, average and current strategies, rank-order and pair-loop leaves"""
    s, dev = device_of(name)
    ids = action_ids(s["nodes"])
    for p in (0, 1):
        for current in (False, True):
            want = restated(name, p, current)
            for sorted_showdowns in (True, False):
                compare(report(dev, p, ids, current=current, sorted_showdowns=sorted_showdowns), want, (name, p, current, sorted_showdowns))
    if name in ("turn_one_hand", "turn_no_opponent"):                # what the case is there for: pairs without a deal, hands that face nothing
        zero = [(restated(name, p)[i]["mass"] == 0).sum() for p in (0, 1) for i in ids]
        assert max(zero) > 0
    dev.close()


@pytest.mark.parametrize("name", ["river_wave_35", "turn_imperfect_recall", "flop_three_rounds"] + SLICES)
def test_both_tree_orders_repeats_and_subsets_give_the_same_bits(name):
    s, dev = device_of(name)
    ids = action_ids(s["nodes"])
    for p in (0, 1):
        for sorted_showdowns in (True, False):
            levels = report(dev, p, ids, sorted_showdowns=sorted_showdowns)
            assert same_reports(report(dev, p, ids, sorted_showdowns=sorted_showdowns), levels), (name, p, "twice")
            with depth_first():
                assert same_reports(report(dev, p, ids, sorted_showdowns=sorted_showdowns), levels), (name, p, sorted_showdowns, "depth first")
                some = ids[::3][::-1]
                part = report(dev, p, some, sorted_showdowns=sorted_showdowns)
            assert list(part) == some and same_reports(part, {i: levels[i] for i in some}), (name, p, "subset, depth first")
            part = report(dev, p, ids[1::2], sorted_showdowns=sorted_showdowns)
            assert same_reports(part, {i: levels[i] for i in ids[1::2]}), (name, p, "subset")
    dev.close()


def test_a_report_has_no_side_effects():
    """the table's cells, rs_best_response_rounds in RS_BR_MAX and RS_BR_AVERAGE and a full-width sweep: the same bits before and after a report"""
    s, dev = device_of("turn_imperfect_recall")
    ids = action_ids(s["nodes"])
    br = lambda mode: dev.table.best_response_rounds(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, mode)
    modes = (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED)
    before = dev.download()
    values = [br(m) for m in modes]
    sweep = [dev.solver().iterate(0), dev.solver().iterate(1)]
    swept = dev.download()
    dev.upload(*s["tables"])
    assert same_tables(dev.download(), before)
    for p in (0, 1):
        for current in (False, True):
            report(dev, p, ids, current=current)
    assert same_tables(dev.download(), before)
    assert all(br(m).tobytes() == v.tobytes() for m, v in zip(modes, values))
    assert [dev.solver().iterate(0), dev.solver().iterate(1)] == sweep
    assert same_tables(dev.download(), swept)
    dev.close()


@pytest.mark.parametrize("name", ["river_lossless_i32", "flop_bucketed_f16"])
def test_trainer_form_and_other_table_types(name):
    """an i32 and a binary16 trainer of test_gpu_br_pinned: the restatement reads the strategies from the downloaded cells; DealTrainer.node_report equals
    InfosetTable.node_report with the trainer's own ranges, board and cluster tables bit for bit; the kept objects do not shrink, and come back after br_release()"""
    tr, tree, nodes, board0, ranges, cids, sizes, dtype = trainer_game(name)
    tr.train(3)
    tr.status()
    R, S = {}, {}
    for nd in tree.action_nodes():
        R[nd.index], S[nd.index] = tr.infosets.download_node(nd.index)
    game = nbr.Game(board0, ranges)
    ids = action_ids(nodes)
    tr.best_response(L.BR_AVERAGE | L.BR_SORTED)
    held = tr.br_bytes()
    assert held > 0
    for current in (False, True):
        sig = nnr.strategies((R, S), current, dtype)
        for p in (0, 1):
            want = nnr.report(nodes, sig.__getitem__, game, cids, p)
            got = tr.node_report(p, ids, current=current)
            compare(got, want, (name, p, current))
            assert tr.br_launches() > 0                             # the level plan ran, on the object best_response() keeps
            assert same_reports(tr.infosets.node_report(tree, board0, ranges[0], ranges[1], cids, p, ids, current=current), got), (name, p, current)
            compare(tr.node_report(p, ids, current=current, sorted_showdowns=False), want, (name, p, current, "pair loop"))
    assert tr.br_bytes() >= held
    held = tr.br_bytes()
    first = tr.node_report(0, ids)
    plain = tr.best_response(L.BR_AVERAGE | L.BR_SORTED)
    tr.br_release()
    assert tr.br_bytes() < held
    assert same_reports(tr.node_report(0, ids), first)
    assert tr.best_response(L.BR_AVERAGE | L.BR_SORTED).tobytes() == plain.tobytes()
    with depth_first():
        tr.br_release()
        assert same_reports(tr.node_report(0, ids), first)
        assert tr.br_launches() == -1
    tr.br_release()
    for nd in tree.action_nodes():
        r, s = tr.infosets.download_node(nd.index)
        assert r.tobytes() == R[nd.index].tobytes() and s.tobytes() == S[nd.index].tobytes()
    tr.destroy()


def test_refused_calls_leave_the_buffer_and_the_table_alone():
    s, dev = device_of("turn_imperfect_recall")
    lib = L.load()
    ids = action_ids(s["nodes"])
    terminal = next(i for i, nd in enumerate(s["nodes"]) if nd["kind"] == "terminal")
    chance = next(i for i, nd in enumerate(s["nodes"]) if nd["kind"] not in ("action", "terminal"))
    b = np.ascontiguousarray(dev.board0, dtype=np.uint8)
    h = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in dev.h]
    keep = [np.ascontiguousarray(dev.cids[r][p], dtype=np.uint32) for r in range(len(dev.cids)) for p in (0, 1)]
    arr = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def size(p, nodes):
        n = np.asarray(nodes, dtype=np.int32)
        return int(lib.rs_node_report_size(dev.tree._h, len(b), len(h[p]), vp(n), len(n), None))

    total = size(0, ids)
    assert total == sum((len(s["nodes"][i]["children"]) + 3) * restated("turn_imperfect_recall", 0)[i]["value"].size for i in ids)
    out = np.full(total + 8, 7.0)
    before = dev.download()

    def call(mode, p, nodes, doubles):
        n = np.asarray(nodes, dtype=np.int32)
        return lib.rs_node_report(dev.table._h, dev.tree._h, vp(b), len(b), vp(h[0]), len(h[0]), vp(h[1]), len(h[1]), arr, len(dev.cids), mode, p, vp(n), len(n), vp(out), doubles)

    avg = L.BR_AVERAGE | L.BR_SORTED
    refused = {
        "RS_BR_MAX": (L.BR_MAX | L.BR_SORTED, 0, ids, len(out)),
        "RS_BR_REAL": (L.BR_MAX | L.BR_REAL, 0, ids, len(out)),
        "RS_BR_AVERAGE | RS_BR_REAL": (L.BR_AVERAGE | L.BR_REAL, 0, ids, len(out)),
        "a terminal node": (avg, 0, ids[:2] + [terminal], len(out)),
        "a chance node": (avg, 0, [chance], len(out)),
        "a repeated id": (avg, 0, ids + ids[:1], len(out)),
        "an id out of range": (avg, 0, [len(s["nodes"])], len(out)),
        "a negative id": (avg, 0, [-1], len(out)),
        "a short buffer": (avg, 0, ids, total - 1),
        "traverser 2": (avg, 2, ids, len(out)),
        "traverser -1": (avg, -1, ids, len(out)),
    }
    for what, args in refused.items():
        assert call(*args) == L.ERR_INVALID, what
        assert (out == 7.0).all(), what
        if "BR" in what:
            assert b"report" in lib.rs_last_error(), what
    for nodes in (ids[:2] + [terminal], [chance], ids + ids[:1], [len(s["nodes"])], [-1]):
        assert size(0, nodes) == 0
    with pytest.raises(rs.RsError):
        report(dev, 0, [terminal])
    with pytest.raises(rs.RsError):
        report(dev, 2, ids)
    assert same_tables(dev.download(), before)
    assert call(avg, 0, ids, len(out)) == L.OK                      # the same arguments with nothing wrong
    assert (out[total:] == 7.0).all() and not (out[:total] == 7.0).any()
    dev.close()

    tr, tree, nodes, board0, ranges, cids, sizes, dtype = trainer_game("river_lossless_i32")
    n = np.asarray(action_ids(nodes), dtype=np.int32)
    buf = np.full(int(lib.rs_node_report_size(tree._h, len(board0), len(ranges[0]), vp(n), len(n), None)), 7.0)
    for mode in (L.BR_MAX, L.BR_MAX | L.BR_REAL | L.BR_SORTED):
        assert lib.rs_deal_trainer_node_report(tr._h, mode, 0, vp(n), len(n), vp(buf), len(buf)) == L.ERR_INVALID
        assert (buf == 7.0).all()
    assert lib.rs_deal_trainer_node_report(tr._h, L.BR_AVERAGE, 0, vp(n), len(n), vp(buf), len(buf) - 1) == L.ERR_INVALID and (buf == 7.0).all()
    tr.destroy()


@pytest.mark.parametrize("order", ["level plan", "depth first"])
def test_a_kept_game_keeps_nothing_of_a_finished_or_refused_report(order):
    """One DealTrainer keeps its prepared game between calls: a best response, a report of two nodes, a report that the library refuses on that kept game (a node id
    out of range) and the best response again -- the same bits and the same launch count as the first.  The 40-node river tree, seven and six hands; in both tree
    orders (the knob is read whenever a workspace is allocated: br_release() inside it)."""
    lib = L.load()
    mask = ab.card_mask("4d5dAs3cKs")
    rng = np.random.Generator(np.random.PCG64(40))
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.choice(len(allh), n, replace=False))] for n in (7, 6)]
    _, tree = rs.build_game_tree(rs.default_flop())
    assert tree.n_nodes == 40
    tr = rs.DealTrainer(tree, [ab.CardAbstraction.init(ranges, mask, 2, None)], ranges, mask, 1 << 12, seed=9, discount_interval=0)
    tr.train(2)
    tr.status()
    ids = [i for i, nd in enumerate(tree.nodes) if nd.kind == L.NODE_ACTION]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    with depth_first() if order == "depth first" else contextlib.nullcontext():
        tr.br_release()
        first = tr.best_response(L.BR_MAX | L.BR_SORTED)
        launches = tr.br_launches()
        assert (launches == -1) == (order == "depth first") and launches != 0
        two = tr.node_report(0, ids[:2])
        assert sorted(two) == ids[:2]
        bad, buf = np.asarray([tree.n_nodes], dtype=np.int32), np.full(64, 7.0)
        with pytest.raises(rs.RsError):                              # past the Python layer's own check of the request: the kept game's br_report refuses
            L.check(lib.rs_deal_trainer_node_report(tr._h, L.BR_AVERAGE | L.BR_SORTED, 0, vp(bad), len(bad), vp(buf), len(buf)))
        assert (buf == 7.0).all()
        with pytest.raises(rs.RsError):
            tr.node_report(0, [tree.n_nodes])
        again = tr.best_response(L.BR_MAX | L.BR_SORTED)
        assert again.tobytes() == first.tobytes() and np.isfinite(first).all()
        assert tr.br_launches() == launches
        assert same_reports(tr.node_report(0, ids[:2]), two)
    tr.destroy()
