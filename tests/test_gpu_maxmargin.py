"""GPU (-m gpu): the max-margin gadget of the full-width solver (rs_range_cfr_set_gadget_kind, rs_range_cfr_gadget_margins), the per-hand root values of the
best-response walk (rs_best_response_hands) and rustsolver_amd.resolve's trunk_rows / best_response_alt / margins, against the numpy restatement tests/np_maxmargin.py.

Teacher-forced like tests/test_gpu_resolve.py: the restatement's tables and gadget rows are uploaded, the device does ONE sweep, and the result is compared with the
restatement's own next state.  Per cell the rule is test_range_cfr_cpu.compare_cells, the gadget's 2 n cells (row 0 of regret and ssum) counted with the table's, at
most 0.5 % of a case's cells differing at all; tests/test_maxmargin_cpu.py holds the restatement's two summation orders to the same rule on the same cases (run here
first, per case).  Cells a sweep must not touch are bit-equal to the upload: row 1 always, row 0 on the resolver's sweep, the cells of dead hands.

gadget_margins() is held to the restatement's margins with the NaN pattern equal and rtol 1e-11 (atol test_np_br_cpu's ATOL), as tests/test_maxmargin_cpu.py holds the
restatement's own two orders.

Shapes: test_resolve_cpu.CASES (what each reaches is listed in tests/test_gpu_resolve.py) and river_hands_300, ranges beyond 256 hands: the second trip of the
one-workgroup kernels' loops over the hands."""
import ctypes as C

import numpy as np
import pytest

import np_maxmargin as nm
import np_node_report as nnr
import np_range_cfr as nrc
import np_resolve as nr
import np_weighted as nw
import rustsolver_amd as rs
from oracle import np_br as nbr
from rustsolver_amd import _lib as L
from rustsolver_amd import resolve
from rustsolver_amd.solver import _range_weights
from test_gpu_br_pinned import GDT, NPDT, depth_first
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, same_tables
from test_locks_cpu import pick_nodes, random_lock
from test_maxmargin_cpu import MM_CASES, best_response_alt, mm_case, mm_inputs, mm_order_check, profile_margins, tree_of
from test_np_br_cpu import ATOL, RTOL
from test_rake_cpu import LOW_CAP_RAKE
from test_range_cfr_cpu import cell_classes, compare_cells, random_tables
from test_resolve_cpu import SAFETY, opponents_best_response, safety_game

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def arm(solver, P, alt, regret, ssum):
    solver.set_gadget(P, alt, kind="maxmargin")
    zr, zs = solver.gadget()
    assert not zr.any() and not zs.any() and zr.shape == (2, len(alt))            # arming zeroes the rows
    solver.set_gadget_rows(regret, ssum)


def same_rows(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def compare_rows(P, p, live, before, got, want, what):
    """the gadget's cells after one sweep of traverser p -> (cells, cells that differ at all)"""
    if p == P:                                                                     # the resolver's sweep leaves them
        assert same_rows(got, before), (what, "the resolver's sweep wrote the gadget rows")
        return 0, 0
    cells = differ = 0
    for g, w, b in zip(got, want, before):
        assert g[1].tobytes() == b[1].tobytes(), (what, "row 1 changed")
        assert g[0, ~live].tobytes() == b[0, ~live].tobytes(), (what, "a dead hand's cell changed")
        d, _ = compare_cells(g[0, live], w[0, live], what)
        cells += d.size
        differ += int((d > 0).sum())
    return cells, differ


def compare_margins(got, want, what):
    assert (np.isnan(got) == np.isnan(want)).all(), (what, "the NaN pattern of the margins")
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-11, atol=ATOL), (what, float(np.abs(got[ok] - want[ok]).max()))


@pytest.mark.parametrize("name", MM_CASES)
def test_one_maxmargin_sweep_equals_the_restatement(name):
    """both resolvers, both traversers, plain and RM+, rank-order and pair-loop leaves, random gadget rows -- and on turn_no_opponent zero rows as well, the uniform branch
    of rho with dead hands beside live ones: tables, gadget rows, value and margins"""
    board0, h, cids, sizes, tree = mm_case(name)
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    c0, d0 = mm_order_check(name, nodes, cids, sizes, game)                        # the restatement's two orders alone stay inside the cap
    assert d0 <= 0.005 * c0, (name, d0, c0)
    dev = Device(board0, h, cids, sizes, tree)
    cells = differ = 0
    configs = [(P, p, rmplus, "random") for P in (0, 1) for p in (0, 1) for rmplus in (False, True)]
    if name == "turn_no_opponent":                                                 # zero rows: norm = 0, rho = 1 / L over the live hands, the dead ones left out of L
        configs += [(1, p, rmplus, "zero") for p in (0, 1) for rmplus in (False, True)]
    for P, p, rmplus, rows in configs:
        rng = np.random.Generator(np.random.PCG64(400 + 4 * P + 2 * p + rmplus + 8 * (rows == "zero")))
        before = random_tables(rng, nodes, sizes)
        alt, gr, gs = mm_inputs(rng, game.n[1 - P], rows)
        want = copy_tables(*before)
        G = dict(resolver=P, alt=alt, regret=gr.copy(), ssum=gs.copy(), margin=None)
        detail = {}
        value = nm.maxmargin_sweep(nodes, want[0], want[1], G, game, cids, p, rmplus, detail=detail)
        live = detail["live"]
        if rows == "zero":
            assert (detail["rho"] == np.where(live, 1.0 / live.sum(), 0.0)).all() and 1 < live.sum() < len(live)
        for sorted_showdowns in (True, False):
            what = (name, P, p, rmplus, rows, sorted_showdowns)
            s = dev.solver(rmplus, sorted_showdowns)
            dev.upload(*before)
            arm(s, P, alt, gr, gs)
            if p == P:
                with pytest.raises(rs.RsError) as e:                       # no sweep of the opponent since arming
                    s.gadget_margins()
                assert e.value.code == L.ERR_INVALID
            got_value = s.iterate(p)
            got, got_rows = dev.download(), s.gadget()
            print(what, "value", got_value, "restated", value)
            assert np.isclose(got_value, value, rtol=RTOL, atol=ATOL), (what, got_value, value)
            c, d, _ = compare_sweep(nodes, game, cids, p, before, got, want, what)
            cg, dg = compare_rows(P, p, live, (gr, gs), got_rows, (G["regret"], G["ssum"]), what)
            cells, differ = cells + c + cg, differ + d + dg
            margins = None
            if p != P:
                margins = s.gadget_margins()
                compare_margins(margins, G["margin"], what)
            if sorted_showdowns:                                           # determinism: the same call from the same state
                dev.upload(*before)
                arm(s, P, alt, gr, gs)
                assert s.iterate(p) == got_value
                assert same_tables(dev.download(), got) and same_rows(s.gadget(), got_rows), what
                assert margins is None or s.gadget_margins().tobytes() == margins.tobytes()
    print(name, "cells", cells, "differ", differ)
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    dev.close()


def test_an_alt_of_1e30_moves_every_cell_by_class():
    """one alt of 1e30 drowns every other term of U: the rows, the margins and the values are compared by class (finite, +inf, -inf, NaN) only"""
    board0, h, cids, sizes, tree = mm_case("river_lanes")
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(411))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = mm_inputs(rng, game.n[0])
    alt[3] = 1e30
    gr[0, 3] = 2.0                                                                 # ... and the hand is chosen
    for p in (0, 1):
        for rmplus in (False, True):
            want = copy_tables(*before)
            G = dict(resolver=1, alt=alt, regret=gr.copy(), ssum=gs.copy(), margin=None)
            value = nm.maxmargin_sweep(nodes, want[0], want[1], G, game, cids, p, rmplus)
            s = dev.solver(rmplus)
            dev.upload(*before)
            arm(s, 1, alt, gr, gs)
            got_value = s.iterate(p)
            rows = s.gadget()
            assert np.isfinite(got_value) == np.isfinite(value) and np.sign(got_value) == np.sign(value) and abs(value) > 1e25
            for g, w in zip(rows, (G["regret"], G["ssum"])):
                assert (cell_classes(g) == cell_classes(w)).all() and g[1].tobytes() == w[1].tobytes()
            if p == 0:
                m = s.gadget_margins()
                assert (np.isnan(m) == np.isnan(G["margin"])).all() and (np.isfinite(m) == np.isfinite(G["margin"])).all() and m[3] > 1e29
                assert (np.abs(rows[0][0]) > 1e25).all() or rmplus                 # every hand's regret moved by -U
    dev.close()


@pytest.mark.parametrize("name", ["turn_imperfect_recall", "river_lanes"])
def test_level_plan_and_depth_first_walk_give_the_same_bits_with_a_maxmargin_gadget(name):
    board0, h, cids, sizes, tree = mm_case(name)
    nodes = tree_of(board0, tree)
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(421))
    before = random_tables(rng, nodes, sizes)
    for P in (0, 1):
        alt, gr, gs = mm_inputs(rng, len(h[1 - P]))
        for rmplus in (False, True):
            for sorted_showdowns in (True, False):
                dev.upload(*before)
                levels = dev.solver(rmplus, sorted_showdowns)
                arm(levels, P, alt, gr, gs)
                v = [levels.iterate(0), levels.iterate(1)]
                assert levels.launches() > 0
                got, rows, margins = dev.download(), levels.gadget(), levels.gadget_margins()
                with depth_first():
                    walk = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns)
                    dev.upload(*before)
                    arm(walk, P, alt, gr, gs)
                    w = [walk.iterate(0), walk.iterate(1)]
                    assert walk.launches() == -1
                    wrows, wmargins = walk.gadget(), walk.gadget_margins()
                assert v == w, (name, P, rmplus, sorted_showdowns, v, w)
                assert same_tables(dev.download(), got) and same_rows(rows, wrows) and margins.tobytes() == wmargins.tobytes(), (name, P, rmplus, sorted_showdowns)
                walk.destroy()
    dev.close()


def test_train_with_dcfr_equals_sweeps_and_ticks_issued_one_by_one_with_a_maxmargin_gadget():
    """3 iterations with DCFR (1.5, 0, 2) against the same sweeps with the table's tick (rs_discount_dcfr) and the gadget's (one f32 multiply per cell of BOTH rows,
    done here)"""
    board0, h, cids, sizes, tree = mm_case("turn_lanes")
    nodes = tree_of(board0, tree)
    dev = Device(board0, h, cids, sizes, tree)
    rng = np.random.Generator(np.random.PCG64(431))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = mm_inputs(rng, len(h[0]))
    for rmplus in (False, True):
        s = dev.solver(rmplus)
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        values = s.train(3, dcfr=True)
        whole, whole_rows, whole_margins = dev.download(), s.gadget(), s.gadget_margins()
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        for t in (1, 2, 3):
            one = [s.iterate(0), s.iterate(1)]
            f = rs.dcfr_factors(1.5, 0.0, 2.0, t)
            dev.table.discount_dcfr(*f)
            G = dict(zip(("regret", "ssum"), s.gadget()))
            nr.gadget_discount(G, *f)
            s.set_gadget_rows(G["regret"], G["ssum"])
        assert same_tables(dev.download(), whole) and one == values.tolist()
        assert same_rows(s.gadget(), whole_rows) and s.gadget_margins().tobytes() == whole_margins.tobytes()
        assert whole_rows[1][1].tobytes() != gs[1].tobytes()                       # the ticks multiplied row 1 as well
        dev.upload(*before)
        arm(s, 1, alt, gr, gs)
        s.train(3)
        assert s.gadget()[1][0].tobytes() != whole_rows[1][0].tobytes() and s.gadget()[1][1].tobytes() == gs[1].tobytes()
    dev.close()


def test_kind_resolve_is_set_gadget_bit_for_bit():
    """rs_range_cfr_set_gadget_kind(RS_GADGET_RESOLVE) on a fresh object against rs_range_cfr_set_gadget on another: tables, rows, values, launches() and bytes; an
    unknown kind is refused and changes nothing; gadget_margins is refused under kind 0"""
    from test_resolve_cpu import gadget_inputs
    board0, h, cids, sizes, tree = mm_case("turn_imperfect_recall")
    nodes = tree_of(board0, tree)
    rng = np.random.Generator(np.random.PCG64(441))
    before = random_tables(rng, nodes, sizes)
    alt, gr, gs = gadget_inputs(rng, len(h[1]))
    out = []
    for by_kind in (False, True):
        dev = Device(board0, h, cids, sizes, tree)
        s = dev.solver()
        dev.upload(*before)
        handle = s._handle(None)
        if by_kind:
            assert L.load().rs_range_cfr_set_gadget_kind(handle, 2, 0, alt.ctypes.data) == L.ERR_INVALID
            assert L.load().rs_range_cfr_set_gadget_kind(handle, -1, 0, alt.ctypes.data) == L.ERR_INVALID
            with pytest.raises(rs.RsError):                                        # the refused calls armed nothing
                s.gadget()
            L.check(L.load().rs_range_cfr_set_gadget_kind(handle, L.GADGET_RESOLVE, 0, alt.ctypes.data))
            s._gadget = (0, alt, L.GADGET_RESOLVE)
        else:
            s.set_gadget(0, alt)
        s.set_gadget_rows(gr, gs)
        values, launches = [], []
        for p in (0, 1, 0, 1):
            values.append(s.iterate(p))
            launches.append(s.launches())
        with pytest.raises(rs.RsError) as e:
            s.gadget_margins()
        assert e.value.code == L.ERR_INVALID
        out.append((values, launches, s.nbytes, dev.download(), s.gadget()))
        dev.close()
    a, b = out
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (a[:3], b[:3])
    assert same_tables(a[3], b[3]) and same_rows(a[4], b[4])


def test_the_launches_of_a_maxmargin_sweep():
    """kind 0: the reach and the TERMINATE leaf (the resolver's sweep), the mass row and the gadget's own node (the opponent's).  Kind 1: rho / M and the per-lane scale,
    the fold and the hand-level update -- as many; the mass row is folded once per arming, in front of the first sweep, and no sweep launches it again"""
    board0, h, cids, sizes, tree = mm_case("turn_imperfect_recall")
    dev = Device(board0, h, cids, sizes, tree)
    s = dev.solver()
    alt = np.zeros(len(h[1]))
    s.set_gadget(0, alt)
    base = []
    for p in (0, 1):
        s.iterate(p)
        base.append(s.launches())
    s.set_gadget(0, alt, kind="maxmargin")
    for p in (0, 1, 0, 1):
        s.iterate(p)
        assert s.launches() == base[p], (p, s.launches(), base)
    dev.close()


# ---- rs_best_response_hands ----------------------------------------------------------------------------------------------------------------------------------------
def tables_of(dtype, rng, nodes, sizes):
    """random tables as the table type stores them"""
    R, S = random_tables(rng, nodes, sizes)
    if dtype == "i32":
        return {i: np.round(x * 100).astype(np.int32) for i, x in R.items()}, {i: np.round(x * 100).astype(np.int32) for i, x in S.items()}
    if dtype == "f16":
        return {i: x.astype(np.float16) for i, x in R.items()}, {i: x.astype(np.float16) for i, x in S.items()}
    return R, S


def hands(dev, p, mode, **kw):
    return dev.table.best_response_hands(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, mode=mode, **kw)


def first_action(nodes):
    return next(i for i, nd in enumerate(nodes) if nd["kind"] == "action")


@pytest.mark.parametrize("dtype", ["f32", "i32", "f16"])
@pytest.mark.parametrize("name", ["river_lanes", "river_wave_35", "turn_imperfect_recall", "turn_no_opponent", "river_hands_300"])
def test_best_response_hands_equals_the_node_report_the_best_response_and_the_restatement(name, dtype):
    board0, h, cids, sizes, tree = mm_case(name)
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    tables = tables_of(dtype, np.random.Generator(np.random.PCG64(451)), nodes, sizes)
    dev = Device(board0, h, cids, sizes, tree, dtype=GDT[dtype])
    dev.upload(*tables)
    root = first_action(nodes)
    for current in (False, True):
        sig = nnr.strategies(tables, current=current, dtype=dtype)
        for sorted_bit in (L.BR_SORTED, 0):
            for p in (0, 1):
                what = (name, dtype, current, sorted_bit, p)
                # RS_BR_AVERAGE: bit-equal to the node report's root rows
                value, mass = hands(dev, p, L.BR_AVERAGE | sorted_bit, current=current)
                rep = dev.table.node_report(dev.tree, board0, h[0], h[1], cids, p, [root], current=current, sorted_showdowns=bool(sorted_bit))[root]
                assert value.tobytes() == rep["value"][0].tobytes() and mass.tobytes() == rep["mass"][0].tobytes(), what
                with depth_first():
                    wv, wm = hands(dev, p, L.BR_AVERAGE | sorted_bit, current=current)
                if sorted_bit:
                    assert wv.tobytes() == value.tobytes() and wm.tobytes() == mass.tobytes(), (what, "the two tree orders")
                for mode, args in ((L.BR_AVERAGE, dict(mode="avg")), (L.BR_MAX, dict(mode="max")), (L.BR_MAX | L.BR_REAL, dict(mode="max", real=True))):
                    value, mass = hands(dev, p, mode | sorted_bit, current=current)
                    total = dev.table.best_response_rounds(dev.tree, board0, h[0], h[1], cids, mode | sorted_bit, current=current)[p]
                    assert abs(value.sum() - total) <= 1e-12 * abs(total), (what, mode, value.sum(), total)
                    if mode != L.BR_AVERAGE and sorted_bit:
                        with depth_first():
                            dv, dm = hands(dev, p, mode | sorted_bit, current=current)
                        assert dv.tobytes() == value.tobytes() and dm.tobytes() == mass.tobytes(), (what, mode, "the two tree orders")
                    if current and dtype == "f16":
                        continue                                                   # (the restatement reads current strategies of f32 and i32 cells)
                    wv, wm = nm.root_hands(nodes, sig.__getitem__, game, cids, p, **args)
                    assert np.allclose(value, wv, rtol=1e-11, atol=ATOL) and np.allclose(mass, wm, rtol=1e-11, atol=ATOL), (what, mode)
    if name == "turn_no_opponent":                                                 # hands that meet no opponent: 0.0 twice
        value, mass = hands(dev, 0, L.BR_MAX | L.BR_REAL)
        assert (value[:2] == 0).all() and (mass[:2] == 0).all() and (mass[2:] > 0).all()
    dev.close()


def test_best_response_hands_with_weights_a_lock_and_rake():
    board0, h, cids, sizes, tree = mm_case("turn_imperfect_recall")
    nodes, game = tree_of(board0, tree), nbr.Game(board0, h)
    rng = np.random.Generator(np.random.PCG64(461))
    tables = random_tables(rng, nodes, sizes)
    sig = nnr.strategies(tables)
    dev = Device(board0, h, cids, sizes, tree)
    dev.upload(*tables)
    w = [rng.random(len(x)) + 0.5 for x in h]
    w[0][2] = 0.0                                                                  # a hand of weight 0 is dropped and put back as 0.0
    kept = [h[0][w[0] != 0], h[1]]
    kept_cids = [[c[0][:, w[0] != 0], c[1]] for c in cids]
    weighted = nw.WeightedGame(board0, kept, (w[0][w[0] != 0], w[1]), "joint")
    node = pick_nodes(nodes)[-1]
    locks = {node: random_lock(np.random.Generator(np.random.PCG64(9)), nodes, game, board0, node, garbage=True)}
    for mode, args in ((L.BR_MAX | L.BR_REAL | L.BR_SORTED, dict(mode="max", real=True)), (L.BR_MAX, dict(mode="max")), (L.BR_AVERAGE, dict(mode="avg"))):
        for p in (0, 1):
            value, mass = hands(dev, p, mode, weights=w, deal="joint")
            wv, wm = nm.root_hands(nodes, sig.__getitem__, weighted, kept_cids, p, **args)
            if p == 0:
                assert value[2] == 0.0 and mass[2] == 0.0
                value, mass = value[w[0] != 0], mass[w[0] != 0]
            assert np.allclose(value, wv, rtol=1e-11, atol=ATOL) and np.allclose(mass, wm, rtol=1e-11, atol=ATOL), ("weighted", mode, p)
            value, mass = hands(dev, p, mode, locks=locks)
            wv, wm = nm.root_hands(nodes, sig.__getitem__, game, cids, p, locks=locks, **args)
            assert np.allclose(value, wv, rtol=1e-11, atol=ATOL) and np.allclose(mass, wm, rtol=1e-11, atol=ATOL), ("locked", mode, p)
            value, mass = hands(dev, p, mode, rake=LOW_CAP_RAKE)
            wv, wm = nm.root_hands(nodes, sig.__getitem__, game, cids, p, rake=LOW_CAP_RAKE, **args)
            free, _ = nm.root_hands(nodes, sig.__getitem__, game, cids, p, **args)
            assert np.allclose(value, wv, rtol=1e-11, atol=ATOL) and np.allclose(mass, wm, rtol=1e-11, atol=ATOL), ("raked", mode, p)
            assert not np.allclose(wv, free, rtol=1e-6)                            # the rake matters
    dev.close()


def test_refused_best_response_hands_calls_leave_the_outputs_alone():
    board0, h, cids, sizes, tree = mm_case("river_lanes")
    nodes = tree_of(board0, tree)
    dev = Device(board0, h, cids, sizes, tree)
    dev.upload(*random_tables(np.random.Generator(np.random.PCG64(471)), nodes, sizes))
    b = np.ascontiguousarray(board0, dtype=np.uint8)
    h0, h1 = (np.ascontiguousarray(x, dtype=np.uint8) for x in h)
    cl = [np.ascontiguousarray(c, dtype=np.uint32) for row in cids for c in row]
    arr = (C.c_void_p * len(cl))(*[k.ctypes.data for k in cl])
    value, mass = np.full(len(h0), 7.25), np.full(len(h0), -3.5)

    def call(mode, traverser, rake=None):
        return L.load().rs_best_response_hands(dev.table._h, dev.tree._h, b.ctypes.data, len(b), h0.ctypes.data, len(h0), h1.ctypes.data, len(h1), arr, len(cids),
                                               _range_weights([None, None], "sequential"), None, rake, mode, traverser, value.ctypes.data, mass.ctypes.data)

    for mode, traverser in ((L.BR_AVERAGE | L.BR_REAL, 0), (2, 0), (L.BR_MAX | 0x800, 0), (L.BR_MAX, 2), (L.BR_MAX, -1)):
        assert call(mode, traverser) == L.ERR_INVALID, (mode, traverser)
        assert (value == 7.25).all() and (mass == -3.5).all()
    bad = L.Rake(-0.5, 3.0)
    assert call(L.BR_MAX, 0, C.byref(bad)) == L.ERR_INVALID and (value == 7.25).all() and (mass == -3.5).all()
    assert call(L.BR_MAX | L.BR_REAL, 0) == L.OK and not (value == 7.25).any() and (mass > 0).all()
    v2, _ = hands(dev, 0, L.BR_MAX | L.BR_REAL, )
    assert v2.tobytes() == value.tobytes()
    only = np.full(len(h0), 1.5)                                                   # mass may be NULL
    assert L.load().rs_best_response_hands(dev.table._h, dev.tree._h, b.ctypes.data, len(b), h0.ctypes.data, len(h0), h1.ctypes.data, len(h1), arr, len(cids),
                                           _range_weights([None, None], "sequential"), None, None, L.BR_MAX | L.BR_REAL, 0, only.ctypes.data, None) == L.OK
    assert only.tobytes() == value.tobytes()
    dev.close()


# ---- the recipe, end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_maxmargin_resolve_end_to_end_equals_the_restatement_and_is_safe():
    """test_resolve_cpu's safety game through prepare -> trunk_rows -> best_response_alt -> a max-margin train -> margins -> graft, on the device and in the restatement:
    trunk 5 plain iterations, 200 iterations with DCFR (1.5, 0, 2).  The device's alt and margins equal the restatement's within 1e-6 (chips per unit mass; the
    trained f32 tables of the two differ by their cells' last bits), and the opponent's best-response value after the graft is not above the trunk's."""
    board0, h, cids, sizes, tree, nodes, game = safety_game()
    P, O = SAFETY["resolver"], 1 - SAFETY["resolver"]
    iterations = 200
    # the restatement
    R, S = nrc.zero_tables(nodes, sizes)
    nrc.train(nodes, R, S, game, cids, SAFETY["trunk_iterations"])
    pre = nr.prepare(nodes, (R, S), board0, h, cids, SAFETY["node"], SAFETY["prefix"], P, game=game)
    want_alt = best_response_alt(pre, (R, S))
    Rs, Ss = nrc.zero_tables(pre["nodes"], sizes)
    nm.maxmargin_train(pre["nodes"], Rs, Ss, nm.new_gadget(P, want_alt), nw.WeightedGame(pre["board"], pre["hands"], pre["weights"], "joint"), pre["clusters"],
                       iterations, dcfr=(1.5, 0.0, 2.0))
    want_margins = profile_margins(pre, Ss, want_alt)
    # the device
    dev = Device(board0, h, cids, sizes, tree)
    br = lambda: dev.table.best_response_rounds(dev.tree, board0, h[0], h[1], cids, L.BR_MAX | L.BR_SORTED, deal="joint")[O]
    trunk = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, deal="joint")
    trunk.train(SAFETY["trunk_iterations"])
    got_before = br()
    prepared = resolve.prepare(dev.table, dev.tree, board0, h, cids, SAFETY["node"], SAFETY["prefix"], P, deal="joint")
    rows = resolve.trunk_rows(dev.table, prepared)
    for k, t in enumerate(prepared.index_map):                                     # the trunk's rows of the subtree's nodes, through index_map
        a, b = rows.download_node(k), dev.table.download_node(int(t))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    alt = resolve.best_response_alt(rows, prepared)
    print("alt", np.abs(alt - want_alt).max())
    assert np.abs(alt - want_alt).max() <= 1e-6
    assert (alt >= prepared.alt - 1e-9).all()                                       # a best response is worth at least the profile's own value
    sub_table = rs.create_infosets(prepared.tree.n_action_nodes, prepared.tree, sizes[prepared.round0:], [1] * len(prepared.clusters), dtype=L.F32)
    solver = rs.RangeCFR(sub_table, prepared.tree, prepared.board, prepared.hands[0], prepared.hands[1], prepared.clusters, weights=prepared.weights, deal="joint")
    solver.set_gadget(P, alt, kind="maxmargin")
    solver.train(iterations, dcfr=True)
    got_margins = resolve.margins(sub_table, prepared, alt)
    print("margins: device min", np.nanmin(got_margins), "restated min", np.nanmin(want_margins), "largest difference", np.nanmax(np.abs(got_margins - want_margins)))
    assert (np.isnan(got_margins) == np.isnan(want_margins)).all() and np.nanmax(np.abs(got_margins - want_margins)) <= 1e-6
    assert np.nanmin(got_margins) >= -1e-5
    resolve.graft(sub_table, dev.table, prepared, P)
    got_after = br()
    print("opponent's best response:", got_before, "->", got_after)
    assert got_after <= got_before
    solver.destroy()
    trunk.destroy()
    dev.close()
