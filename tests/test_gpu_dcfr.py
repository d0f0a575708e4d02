"""GPU (-m gpu): Discounted CFR.  The standalone three-factor sweep (rs_discount_dcfr) against ten lines of numpy at the numeric edges; rs_train_dcfr fused (the tick
applied inside the next sweeps' row loads), unfused (the sweep between iterations) and the numpy walk (oracle/np_walk.iterate_lanes + the same ten lines) against each
other, bit for bit; split runs; the solvers that cannot fuse; a host-driven loop with a held pair sweep in front of the tick; kept shadow records under unequal factors;
the deal trainer's ticks.  The library takes its factors as floats, so the reference takes them from rs_dcfr_factors (pinned on the CPU side, test_dcfr_cpu.py)."""
import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from oracle import np_restate as npr
from oracle import np_walk as npw
from test_gpu_walk_restated import DTYPES, assert_no_nan_strategy, assert_same, edge_float, edge_i32, edge_utils, same_tables

pytestmark = pytest.mark.gpu

F32 = np.float32
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
DCFR = (1.5, 0.0, 2.0)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: these tests need a real MI355X (there is no CPU fallback)")


def np_discount3(tab, f, dtype):
    """the tick: regrets > 0 times f[0], the others times f[1], strategy sums times f[2]; i32: ((x as f32) * d) as i32; binary16: rounded once"""
    f = np.asarray(f, dtype=F32)
    with np.errstate(all="ignore"):
        for idx, (R, S) in list(tab.items()):
            r = (R.astype(F32) * np.where(R > 0, f[0], f[1]).astype(F32)).astype(F32)
            s = (S.astype(F32) * f[2]).astype(F32)
            if dtype == "i32":
                tab[idx] = (npr.rust_f32_as_i32(r), npr.rust_f32_as_i32(s))
            else:
                tab[idx] = (npr.round_f16(r), npr.round_f16(s)) if dtype == "f16" else (r, s)


# ---- 1. the standalone sweep ------------------------------------------------------------------------------------------------------------------

def edge_cells(rng, dtype, A, n):
    if dtype == "i32":
        special = np.array([0, 1, -1, 2**24 + 1, 2**24 - 1, -(2**24) - 1, -(2**24) + 1, I32_MIN, I32_MAX, I32_MAX - 64, I32_MIN + 64, 3, -3], dtype=np.int64)
        X = rng.integers(I32_MIN, I32_MAX, size=(A, n), endpoint=True)
        pick = rng.integers(0, 2 * len(special), size=(A, n))
        return np.where(pick < len(special), special[np.minimum(pick, len(special) - 1)], X).astype(np.int32)
    half = dtype == "f16"
    top, tiny = (65504.0, 2.0**-24) if half else (3.4028234e38, 1e-45)
    special = np.array([0.0, -0.0, 1.0, -1.0, top, -top, tiny, -tiny, 3 * tiny, np.inf, -np.inf, np.nan, 0.333, -1234.5], dtype=F32)
    X = (rng.uniform(-1, 1, size=(A, n)) * 1000).astype(F32)
    pick = rng.integers(0, 2 * len(special), size=(A, n))
    X = np.where(pick < len(special), special[np.minimum(pick, len(special) - 1)], X).astype(F32)
    return npr.round_f16(X) if half else X


@pytest.mark.parametrize("layout", ["plain", "tiled64"])
@pytest.mark.parametrize("dtype", ["i32", "f32", "f16"])
def test_discount_dcfr_against_numpy(dtype, layout, monkeypatch):
    """two nodes (2 x 1 021 and 3 x 7 001 lanes: 5 792 vectors per array, more than one 4 096-vector trip and no multiple of it) whose cells include 0, +-1, +-2^24 +- 1,
    INT32_MIN / MAX, +-0.0, subnormals, +-inf, NaN and the largest finite value; factors (1, 0, 0.5), DCFR's own at p = 3, and (0.75, 0.75, 0.75) = rs_discount(0.75)"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    rng = np.random.Generator(np.random.PCG64(7))
    table = rs.InfosetTable.create([(2, 1021, 1, 0, 0), (3, 7001, 1, 1, 0)], DTYPES[dtype])
    twin = rs.InfosetTable.create([(2, 1021, 1, 0, 0), (3, 7001, 1, 1, 0)], DTYPES[dtype])
    assert (table.tile_lanes(1) == 64) == (layout == "tiled64")
    tab = {}
    for idx, (A, n) in enumerate([(2, 1021), (3, 7001)]):
        R, S = edge_cells(rng, dtype, A, n), edge_cells(rng, dtype, A, n)
        table.upload_node(idx, R, S)
        twin.upload_node(idx, R, S)
        tab[idx] = (R.copy(), S.copy())
    for f in [(1.0, 0.0, 0.5), tuple(rs.dcfr_factors(*DCFR, 3)), (0.75, 0.75, 0.75)]:
        table.discount_dcfr(*f)
        np_discount3(tab, f, dtype)
        same_tables(table, tab, "factors %r" % (f,))
        if f[0] == f[1] == f[2]:
            twin.discount(f[0])   # three equal factors ARE rs_discount
        else:
            twin.discount_dcfr(*f)
    for i in tab:
        for a, b in zip(table.download_node(i), twin.download_node(i)):
            assert_same(a, b, "discount_dcfr(d, d, d) against discount(d), node %d" % i)
    table.destroy()
    twin.destroy()


# ---- the lane solvers ---------------------------------------------------------------------------------------------------------------------------

def plain_i32(rng, A, n):
    return rng.integers(-10**6, 10**6, size=(A, n)).astype(np.int32), rng.integers(0, 10**6, size=(A, n)).astype(np.int32)


def plain_float(half):
    def init(rng, A, n):
        R, S = rng.uniform(-1000, 1000, size=(A, n)).astype(F32), rng.uniform(0, 1000, size=(A, n)).astype(F32)
        return (npr.round_f16(R), npr.round_f16(S)) if half else (R, S)
    return init


CASES = {   # dtype, mode, rmplus, scale, init, leaf magnitude
    "i32-clamp": ("i32", "clamp", False, 100.0, plain_i32, 2e4),
    "i32-wrap": ("i32", "wrap", False, 10000.0, plain_i32, 2e2),
    "f32": ("f32", "clamp", False, 1.0, plain_float(False), 50.0),
    "f16": ("f16", "clamp", False, 1.0, plain_float(True), 50.0),
    "f32-rmplus": ("f32", "clamp", True, 1.0, plain_float(False), 50.0),
}


class Lanes:
    """a lane solver and its numpy twin: the table, both traversers' LEAF_UTIL rows, the sweep counter of the sampling seeds"""

    def __init__(self, case, boards, C, seed, graph=False, forms=None, opp="full", prune=False, fuse=1, options=None, chance="pass", init=None, utils=None):
        self.dtype, self.mode, self.rmplus, self.scale, init0, mag = CASES[case]
        init = init or init0
        utils = utils or (lambda rng, n: (rng.uniform(-1, 1, size=n) * mag).astype(F32))
        self.boards, self.C, self.seed, self.prune, self.opp, self.chance = boards, C, seed, prune, opp, chance
        rng = np.random.Generator(np.random.PCG64(seed))
        n_act, self.tree = rs.build_game_tree(options or rs.default_flop())
        self.nodes = npw.tree_from_records(self.tree.nodes)
        self.table = rs.create_infosets(n_act, self.tree, [C], boards, DTYPES[self.dtype])
        self.tab = {}
        for nd in self.tree.action_nodes():
            R, S = init(rng, nd.n_children, self.table.lanes(nd.index))
            self.table.upload_node(nd.index, R, S)
            self.tab[nd.index] = (R.copy(), S.copy())
        self.ln, lg = [{}, {}], [{}, {}]
        for p in (0, 1):
            for i, d in enumerate(self.nodes):
                if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED":
                    par = self.nodes[d["parent"]]
                    buf = utils(rng, self.table.lanes(par["index"]))
                    self.ln[p][i] = ("util", buf)
                    lg[p][i] = (rs.LEAF_UTIL, self.table.lane_buffer(par["index"], 1, buf))
        m = (rs.UPD_WRAP_I32 if self.mode == "wrap" else rs.UPD_CLAMP_I64) | (rs.UPD_PRUNE if prune else 0) | (rs.UPD_RMPLUS if self.rmplus else 0)
        self.tr = rs.MCCFRTrainer(self.tree, self.table, lg[0], leaves_p1=lg[1], scale=self.scale, mode=m, chance_mode=rs.CHANCE_ENUM if chance == "enum" else rs.CHANCE_PASS,
                                  use_graph=graph, fuse_subtrees=fuse, opp_mode=rs.OPP_SAMPLE if opp == "sample" else rs.OPP_FULL, sample_seed=seed, forms=forms)
        self.sweeps = 0

    def np_sweep(self, player):
        if self.dtype != "i32":
            assert_no_nan_strategy(self.tab, "before sweep %d" % self.sweeps)
        u = npw.iterate_lanes(self.nodes, self.tab, self.ln[player], self.boards, self.C, player, scale=self.scale, mode=self.mode, prune=self.prune, rmplus=self.rmplus,
                              dtype=self.dtype, chance=self.chance, opp=self.opp, seed=npr.sweep_seed(self.seed, self.sweeps))
        self.sweeps += 1
        return u

    def np_train(self, iters, abg=DCFR, interval=1, cap=None, t0=0):
        t = t0
        for _ in range(iters):
            self.np_sweep(0)
            self.np_sweep(1)
            t += 1
            if (cap is None or t <= cap) and t % interval == 0:
                np_discount3(self.tab, rs.dcfr_factors(*abg, t // interval), self.dtype)

    def check(self, what, plain_pair=True):
        same_tables(self.table, self.tab, what)
        if plain_pair:   # the root utilities of one more plain iteration: what the trained tables give back (rs_train_dcfr takes no root-utility pointer)
            for p in (0, 1):
                assert_same(self.tr.iterate(p, want_root_util=True), self.np_sweep(p), "%s: root util p=%d after the loop" % (what, p))
            same_tables(self.table, self.tab, what + " + one plain iteration")

    def close(self):
        self.tr.destroy()
        self.table.destroy()


# ---- 2. fused = unfused = numpy -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph,layout", [(False, "plain"), (True, "plain"), (False, "tiled64"), (True, "tiled64")])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_unfused_numpy(case, graph, layout, monkeypatch):
    """river tree, 3 boards x 250 clusters (750 lanes: 188 vectors, one workgroup), five iterations with a tick after every one and after every second one"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    for interval in (1, 2):
        for fused in (True, False):
            x = Lanes(case, [3], 250, 100 + interval, graph=graph)
            x.tr.train_dcfr(5, *DCFR, interval=interval, fused=fused)
            assert x.tr.dcfr_fused == fused
            x.np_train(5, interval=interval)
            x.check("%s interval=%d fused=%s" % (case, interval, fused))
            x.close()


@pytest.mark.parametrize("case", ["i32-clamp", "i32-wrap", "f32", "f16"])
def test_fused_edges_and_first_iteration(case, monkeypatch):
    """1 021 lanes of edge cells (i32: INT32_MIN / MAX, +-2^24-sized values and beyond; floats: subnormals, -0.0, NaN cells) with RS_JIT_MAX_BLOCKS = 2 (several trips
    per workgroup).  The first fused iteration has nothing pending: cells beyond 2^24 must come out as the plain sweeps leave them, not as ((x as f32) * 1.0) as i32;
    then two more iterations whose ticks are applied on load, and the last tick swept.  Factors (1, 0, 0.5): positive regrets keep every bit."""
    monkeypatch.setenv("RS_JIT_MAX_BLOCKS", "2")
    half = case == "f16"
    init = edge_i32 if case.startswith("i32") else edge_float(half, big_rows=False)
    utils = (lambda rng, n: edge_utils(rng, n)) if case.startswith("i32") else None
    abg = (float("inf"), float("-inf"), 1.0)
    for first in (1, 3):
        x = Lanes(case, [1], 1021, 7, init=init, utils=utils)
        x.tr.train_dcfr(first, *abg, cap=0 if first == 1 else None, fused=True)
        assert x.tr.dcfr_fused
        x.np_train(first, abg=abg, cap=0 if first == 1 else None)
        x.check("%s: %d fused iteration(s)" % (case, first), plain_pair=False)
        if first == 1 and case.startswith("i32"):
            big = sum(int((np.abs(R.astype(np.int64)) > 2**24).sum()) for R, _ in x.tab.values())
            assert big > 1000   # the input condition: such cells exist after the sweep, and (same_tables above) hold what the plain sweeps wrote
        x.close()


# ---- 3. split runs -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["i32-clamp", "f16"])
@pytest.mark.parametrize("fused", [True, False])
def test_split_runs(case, fused):
    """2 + 3 iterations with t0 = 2 equal 5 (interval 2: the tick after iteration 2 ends the first call, pending in the fused form and swept before it returns)"""
    x = Lanes(case, [3], 250, 31)
    x.tr.train_dcfr(2, *DCFR, interval=2, fused=fused)
    x.tr.train_dcfr(3, *DCFR, interval=2, t0=2, fused=fused)
    assert x.tr.dcfr_fused == fused
    x.np_train(5, interval=2)
    x.check("%s split 2 + 3" % case)
    x.close()


# ---- 4. the solvers that cannot fuse --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["prune", "sample", "three-street-enum", "level-plan"])
def test_fallbacks_sweep_between_iterations(which):
    kw = {"prune": dict(prune=True), "sample": dict(opp="sample"), "three-street-enum": dict(options=rs.three_street_options(), chance="enum"), "level-plan": dict(fuse=0)}[which]
    boards, C = ([1, 2, 6], 12) if which == "three-street-enum" else ([3], 250)
    x = Lanes("i32-clamp", boards, C, 41, **kw)
    x.tr.train_dcfr(3, *DCFR, fused=True)   # asked for, not possible: the ticks are swept
    assert not x.tr.dcfr_fused
    x.np_train(3)
    x.check(which)
    x.close()


@pytest.mark.parametrize("graph", [False, True])
def test_paired_solver_trains_like_the_unpaired_one(graph):
    a = Lanes("i32-clamp", [3], 250, 43, graph=graph)
    b = Lanes("i32-clamp", [3], 250, 43, graph=graph, forms={"pair_sweeps": L.FORM_OFF})
    assert a.tr.paired and not b.tr.paired
    for x in (a, b):
        x.tr.train_dcfr(4, *DCFR, fused=True)
        assert x.tr.dcfr_fused
        x.np_train(4)
    assert a.tr.paired and a.tr.n_launches(0) + a.tr.n_launches(1) == 1   # still one pair launch per iteration ...
    lib = L.load()
    for x in (a, b):   # ... and a plain pair of rs_iterate calls (a: held, then one pair launch) still matches
        L.check(lib.rs_iterate(x.tr._h, 0, None))
        L.check(lib.rs_iterate(x.tr._h, 1, None))
        x.np_sweep(0)
        x.np_sweep(1)
        x.check("paired" if x is a else "unpaired")
        x.close()


# ---- 5. a host-driven loop ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["i32-clamp", "f32"])
def test_host_driven_loop_and_a_held_sweep_in_front_of_the_tick(case):
    """rs_iterate x 2 + rs_discount_dcfr per iteration is rs_train_dcfr's schedule; and with the tick BETWEEN the two sweeps of a paired solver the held traverser-0 sweep
    must be on the stream before the discount"""
    x = Lanes(case, [3], 250, 47)
    y = Lanes(case, [3], 250, 47)
    assert x.tr.paired
    lib = L.load()
    for t in range(1, 4):
        L.check(lib.rs_iterate(x.tr._h, 0, None))
        L.check(lib.rs_iterate(x.tr._h, 1, None))
        x.table.discount_dcfr(*rs.dcfr_factors(*DCFR, t))
    y.tr.train_dcfr(3, *DCFR, fused=True)
    x.np_train(3)
    y.np_train(3)
    x.check("host-driven", plain_pair=False)
    y.check("rs_train_dcfr", plain_pair=False)
    for t in range(1, 3):   # sweep 0 (held), tick, sweep 1
        f = rs.dcfr_factors(*DCFR, t)
        L.check(lib.rs_iterate(x.tr._h, 0, None))
        x.table.discount_dcfr(*f)
        L.check(lib.rs_iterate(x.tr._h, 1, None))
        x.np_sweep(0)
        np_discount3(x.tab, f, x.dtype)
        x.np_sweep(1)
    x.check("held sweep in front of the tick")
    x.close()
    y.close()


# ---- 6. kept shadow records -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kept", [L.FORM_ON, L.FORM_OFF])
def test_kept_records_under_unequal_factors(kept):
    """a one-round deal solver whose traverser nodes have 16 385 clusters (direct rows, kept records), 4 096 deals, inside rs_solver_training_loop: ticks with unequal
    factors write the working copy back, sweep the table and have the records rebuilt before the next sweep"""
    n_deals, seed, sizes = 4096, 59, [(16385, 16385)]
    rng = np.random.Generator(np.random.PCG64(seed))
    n_act, tree = rs.build_game_tree(rs.default_flop())
    nodes = npw.tree_from_records(tree.nodes)
    table = rs.create_infosets(n_act, tree, sizes, [1], rs.I32)
    tab = {}
    for nd in tree.action_nodes():
        R, S = plain_i32(rng, nd.n_children, sizes[0][nd.player])
        table.upload_node(nd.index, R, S)
        tab[nd.index] = (R.copy(), S.copy())
    cidx = {(0, p): rng.integers(0, sizes[0][p], size=n_deals).astype(np.uint32) for p in (0, 1)}
    buf = (rng.uniform(-1, 1, size=n_deals) * 2e4).astype(F32)
    dbuf = rs.deal_buffer(table, n_deals, buf)
    term = [i for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"]
    tr = rs.MCCFRTrainer(tree, table, {i: (rs.LEAF_UTIL, dbuf) for i in term}, scale=100.0, mode=rs.UPD_CLAMP_I64, fuse_subtrees=1, deals=cidx, opp_mode=rs.OPP_SAMPLE,
                         sample_seed=seed, forms={"kept_records": kept})
    assert tr.delta_rows
    ln = {i: ("util", buf) for i in term}
    tr.training_loop(True)
    k = 0
    for t in range(1, 4):
        for player in (0, 1):
            tr.iterate(player)
            npw.iterate_deals(nodes, tab, ln, cidx, player, scale=100.0, mode="clamp", dtype="i32", opp="sample", seed=npr.sweep_seed(seed, k))
            k += 1
        f = rs.dcfr_factors(*DCFR, t)
        table.discount_dcfr(*f)
        np_discount3(tab, f, "i32")
    tr.training_loop(False)
    same_tables(table, tab, "kept_records=%d" % kept)
    tr.destroy()
    table.destroy()


# ---- 7. the deal trainer -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["i32", "f32"])
def test_deal_trainer_ticks(dtype):
    """a river trainer, 4 096 deals per batch, discount_interval = one batch, six batches replayed deal for deal through np_walk.iterate_deals with the three-factor tick
    where train() ticks (t > threshold: after batches 2, 4 and 6, p = t / interval); then set_dcfr off: the reference's tick again, against an untouched trainer"""
    mask = ab.card_mask("4d5dAs3cKs")
    hands = ab.random_range(mask)
    n_deals, seed = 4096, 19
    n_act, tree = rs.build_game_tree(rs.default_flop())
    nodes = npw.tree_from_records(tree.nodes)
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, 2, None)]
    scale = 100.0 if dtype == "i32" else 0.5
    mk = lambda: rs.DealTrainer(tree, card_abs, [hands, hands], mask, n_deals, seed=seed, discount_interval=n_deals, discount_cap=10**9, prune_threshold=None, scale=scale,
                                dtype=DTYPES[dtype], mode=rs.UPD_CLAMP_I64)
    tr, ref = mk(), mk()
    tr.set_dcfr(*DCFR)
    sizes = [(a.get_size(0), a.get_size(1)) for a in card_abs]
    rng = np.random.Generator(np.random.PCG64(5))
    tab = {}
    for nd in tree.action_nodes():
        R, S = (plain_i32 if dtype == "i32" else plain_float(False))(rng, nd.n_children, sizes[0][nd.player])
        for x in (tr, ref):
            x.infosets.upload_node(nd.index, R, S)
        tab[nd.index] = (R.copy(), S.copy())
    term = [i for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"]
    t, threshold, k, ticks = 0, n_deals, 0, 0
    for b in range(6):
        tr.train(1)
        cidx = {(0, p): tr.clusters(0, p) for p in (0, 1)}
        leaves = {i: ("sign", tr.signs()) for i in term}
        for player in (0, 1):
            npw.iterate_deals(nodes, tab, leaves, cidx, player, scale=scale, mode="clamp", dtype=dtype, opp="sample", seed=npr.sweep_seed(seed, k))
            k += 1
        t += n_deals
        if t > threshold:
            np_discount3(tab, rs.dcfr_factors(*DCFR, t // n_deals), dtype)
            threshold = t + n_deals
            ticks += 1
        same_tables(tr.infosets, tab, "batch %d" % b)
    assert ticks == 3 and tr.iterations == 6 * n_deals
    # back to cfr.rs:248-261: both trainers from the same table, two more batches each (one tick)
    ref.train(6)       # the untouched trainer catches up on the deal numbers (its own ticks on its own table), then takes the other's table
    for nd in tree.action_nodes():
        ref.infosets.upload_node(nd.index, *tab[nd.index])
    tr.set_dcfr(enable=False)
    tr.train(2)
    ref.train(2)
    for nd in tree.action_nodes():
        for a, c in zip(tr.infosets.download_node(nd.index), ref.infosets.download_node(nd.index)):
            assert_same(a, c, "set_dcfr(NULL) against an untouched trainer, node %d" % nd.index)
