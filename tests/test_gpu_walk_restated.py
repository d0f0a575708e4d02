"""GPU (-m gpu): the device's lane and deal sweeps against the numpy restatement of the walks (oracle/np_walk.py), with no C oracle in
between, at the numeric edges where kernels go wrong: i32 regrets at INT32_MIN / INT32_MAX and around the prune threshold, LEAF_UTIL deltas
that straddle 2^31 and 2^32 in waves that are all small, all large or mixed (the wave-uniform fast path of visit_i32), NaN and +-inf
utilities, zero-probability opponent actions, all-non-positive rows; binary16 rows that overflow to inf, subnormal halves, -0.0 and NaN
reaching the RM+ floor, f32 near FLT_MAX; lane counts that are no multiple of 4 or 64, fused and level plans, both lane-fan forms, graph
replay, 64-lane table tiles, the deal-sweep forms, a round beyond 16 384 clusters, and DealTrainer batches replayed deal for deal.
Bar: bit-equal, every NaN counted as one value.

Which kernel a lane case reaches.  run_lanes reads the root utilities and every node after each single sweep.  On a paired solver (river tree, CHANCE_PASS, fuse=1:
rs_kernel_forms.pair_sweeps, the default) rs_iterate(s, 0) only HOLDS the sweep, and the read that follows settles it as a plain traverser-0 sweep; traverser 1 then finds
nothing held and runs plain as well.  So run_lanes pins the plain kernels and the settle path (worth pinning; it returns tr.paired, and test_i32_edges_river asserts that its
fuse=1 solvers ARE paired ones driven this way), and never a pair launch.  The pair kernel is pinned by run_pair_lanes and the test_pair_* cases below: rs_iterate(h, 0, u0),
rs_iterate(h, 1, u1) with nothing in between, tr.paired and the launch count asserted, and only then the reads."""
import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from oracle import np_restate as npr
from oracle import np_walk as npw
from rustsolver_amd import abstraction as ab

pytestmark = pytest.mark.gpu

F32 = np.float32
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
DTYPES = {"i32": rs.I32, "f32": rs.F32, "f16": rs.F16}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: these tests need a real MI355X (there is no CPU fallback)")


def canon(x):
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.int32:
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    else:
        bad = np.nonzero(canon(got) != canon(want))[0]
    assert bad.size == 0, "%s: %d/%d values differ, first at %d: %r vs %r" % (what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]],
                                                                           want.reshape(-1)[bad[0]])


def same_tables(table, tab, what="", before=None):
    for idx, (R, S) in tab.items():
        r, s = table.download_node(idx)
        for x, X, nm in ((r, R, "regrets"), (s, S, "strategy sums")):
            old = "" if before is None else " (before the sweep: %r)" % (before[idx][0 if nm == "regrets" else 1].reshape(-1)[
                np.nonzero(canon(x) != canon(X))[0][:1]] if X.dtype != np.int32 else "")
            assert_same(x, X, "%s %s of node %d%s" % (what, nm, idx, old))


def edge_i32(rng, A, n):
    """regrets: half uniform over all of i32, half INT32_MIN / INT32_MAX / the prune threshold and one below / 0 / +-1; every 5th lane all
    non-positive (uniform strategy).  Strategy sums: full range with saturating values."""
    special = np.array([I32_MIN, I32_MAX, -10_000_000, -10_000_001, 0, -1, 1], dtype=np.int64)
    R = rng.integers(I32_MIN, I32_MAX, size=(A, n), endpoint=True)
    pick = rng.integers(0, 2 * len(special), size=(A, n))
    R = np.where(pick < len(special), special[np.minimum(pick, len(special) - 1)], R)
    R[:, ::5] = -np.abs(R[:, ::5])
    S = rng.integers(I32_MIN, I32_MAX, size=(A, n), endpoint=True)
    S[:, ::7] = I32_MAX
    S[:, 3::7] = I32_MAX - 50
    return R.astype(np.int32), S.astype(np.int32)


def edge_utils(rng, n):
    """LEAF_UTIL values per lane in blocks of 1 024: |u| < 1e4 (deltas far below 2^31), |u| < 2e7 (scale 100: deltas up to 4e9, straddling
    2^31, below 2^32), |u| up to 1e8 (beyond 2^32), then the three mixed lane by lane with NaN and +-inf sprinkled in"""
    u = np.empty(n, dtype=F32)
    blk = np.arange(n) // 1024
    mix = rng.integers(0, 3, size=n)
    kind = np.where(blk < 3, blk, mix)
    mag = np.array([1e4, 2e7, 1e8], dtype=np.float64)[kind]
    u[:] = rng.uniform(-1, 1, size=n) * mag
    tail = np.nonzero(blk >= 3)[0]
    u[tail[::97]] = np.nan
    u[tail[13::89]] = np.inf
    u[tail[29::83]] = -np.inf
    return u


def lane_leaves(table, tree, nodes, make):
    """{node id: (kind, device buffer)} and the numpy twin; make(round_idx, lanes) -> (kind, float32 array)"""
    lg, ln = {}, {}
    for i, d in enumerate(nodes):
        if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED":
            parent = nodes[d["parent"]]
            kind, buf = make(parent["round_idx"], table.lanes(parent["index"]))
            lg[i] = (rs.LEAF_UTIL if kind == "util" else rs.LEAF_SIGN, table.lane_buffer(parent["index"], 1, buf))
            ln[i] = (kind, buf)
    return lg, ln


def run_lanes(options, boards, C, init, make_leaves, mode="clamp", prune=False, rmplus=False, dtype="i32", chance="pass", opp="full",
              seed=1, iters=3, scale=100.0, fuse=1, graph=False, forms=None, players=(0, 1)):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_act, tree = rs.build_game_tree(options)
    nodes = npw.tree_from_records(tree.nodes)
    table = rs.create_infosets(n_act, tree, [C], boards, DTYPES[dtype])
    tab = {}
    for nd in tree.action_nodes():
        R, S = init(rng, nd.n_children, table.lanes(nd.index))
        table.upload_node(nd.index, R, S)
        tab[nd.index] = (R.copy(), S.copy())
    l0 = lane_leaves(table, tree, nodes, lambda r, n: make_leaves(rng, r, n))
    l1 = lane_leaves(table, tree, nodes, lambda r, n: make_leaves(rng, r, n))
    m = (rs.UPD_WRAP_I32 if mode == "wrap" else rs.UPD_CLAMP_I64) | (rs.UPD_PRUNE if prune else 0) | (rs.UPD_RMPLUS if rmplus else 0)
    tr = rs.MCCFRTrainer(tree, table, l0[0], leaves_p1=l1[0], scale=scale, mode=m, chance_mode=rs.CHANCE_ENUM if chance == "enum" else rs.CHANCE_PASS,
                         use_graph=graph, fuse_subtrees=fuse, opp_mode=rs.OPP_SAMPLE if opp == "sample" else rs.OPP_FULL, sample_seed=seed, forms=forms)
    paired = tr.paired   # a paired solver's sweeps below are held, then settled as plain sweeps by the read: see the module docstring
    k = 0
    for it in range(iters):
        for player in players:
            before = {i: (R.copy(), S.copy()) for i, (R, S) in tab.items()}
            got = tr.iterate(player, want_root_util=True)
            want = npw.iterate_lanes(nodes, tab, (l0, l1)[player][1], boards, C, player, scale=scale, mode=mode, prune=prune, rmplus=rmplus,
                                     dtype=dtype, chance=chance, opp=opp, seed=npr.sweep_seed(seed, k))
            k += 1
            same_tables(table, tab, "it=%d p=%d" % (it, player), before)
            assert_same(got, want, "root util it=%d p=%d" % (it, player))
    return paired


# ---- i32 tables through whole walks --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+prune", "clamp+rmplus", "clamp+rmplus+prune"])
@pytest.mark.parametrize("fuse,graph,layout", [(1, False, "plain"), (0, False, "plain"), (1, True, "tiled64"), (0, True, "tiled64")])
def test_i32_edges_river(mode, fuse, graph, layout, monkeypatch):
    """the river tree over 4 099 lanes (no multiple of 4 or 64) with edge regrets and LEAF_UTIL leaves whose deltas straddle 2^31 and 2^32"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    paired = run_lanes(rs.default_flop(), [1], 4099, edge_i32, lambda rng, r, n: ("util", edge_utils(rng, n)), mode=mode.split("+")[0], prune="prune" in mode,
                       rmplus="rmplus" in mode, scale=10000.0 if mode == "wrap" else 100.0, fuse=fuse, graph=graph, seed=11 + fuse)
    assert paired == (fuse == 1)   # fuse=1: a paired solver whose held sweeps the per-sweep reads settled as plain ones (the pair launch itself: test_pair_i32_edges_river)


@pytest.mark.parametrize("fuse", [1, 0])
def test_i32_edges_river_sampled(fuse):
    run_lanes(rs.default_flop(), [3], 1367, edge_i32, lambda rng, r, n: ("util", edge_utils(rng, n)), mode="clamp", prune=True, opp="sample",
              fuse=fuse, seed=21)


@pytest.mark.parametrize("boards,C,lane_fan", [([1, 2, 6], 12, 2), ([1, 2, 6], 12, 1), ([1, 3, 3], 9, 1), ([1, 1, 1], 37, 2)])
@pytest.mark.parametrize("fuse", [1, 0])
def test_i32_edges_three_streets_enum(boards, C, lane_fan, fuse):
    """ENUM chance (reach x 1/fan down, summed util up, child lane b * fan + d) through the expand step inside the subtree kernel (lane_fan 2,
    n_clusters % 4 == 0) and through separate expand launches (1)"""
    run_lanes(rs.three_street_options(), boards, C, edge_i32, lambda rng, r, n: ("util", rng.uniform(-2e7, 2e7, size=n).astype(F32)), mode="clamp",
              prune=True, chance="enum", fuse=fuse, forms={"lane_fan": lane_fan}, seed=31, iters=2)


# ---- float tables ------------------------------------------------------------------------------------------------------------

def edge_float(half, big_rows=True):
    def init(rng, A, n):
        """blocks of 16 lanes: near the largest finite value (big_rows), subnormal halves and -0.0, NaN cells, ordinary values"""
        blk = (np.arange(n) // 16) % 4
        top = 65504.0 if half else 3.4e38
        R = rng.uniform(-1000, 1000, size=(A, n)).astype(F32)
        S = rng.uniform(0, 1000, size=(A, n)).astype(F32)
        big = (blk == 0) & big_rows
        R[:, big] = (rng.choice([-1.0, 1.0], size=(A, int(big.sum()))) * top * rng.uniform(0.9, 1.0, size=(A, int(big.sum())))).astype(F32)
        S[:, big] = top * F32(0.999)
        tiny = blk == 1
        R[:, tiny] = (rng.integers(-1023, 1024, size=(A, int(tiny.sum()))) * 2.0**-24).astype(F32)
        R[:, np.nonzero(tiny)[0][::3]] = F32(-0.0)
        S[:, tiny] = F32(-0.0)
        nan = blk == 2
        R[0, nan] = np.nan
        if half:
            R, S = npr.round_f16(R), npr.round_f16(S)
        return R, S
    return init


def float_utils(half, big=True):
    def make(rng, r, n):
        blk = (np.arange(n) // 16) % 4
        u = rng.uniform(-500, 500, size=n).astype(F32)
        if big:   # utilities that overflow a row near the largest finite value
            u[blk == 0] = (rng.uniform(-1, 1, size=int((blk == 0).sum())) * (6e4 if half else 3e38)).astype(F32)
        u[blk == 1] = (rng.uniform(-1, 1, size=int((blk == 1).sum())) * 3e-5).astype(F32)
        u[np.nonzero(blk == 1)[0][::5]] = F32(-0.0)
        u[(blk == 2) & (np.arange(n) % 3 == 0)] = np.nan
        return "util", u
    return make


# One traverser sweep per fresh table: a regret that overflows to +inf makes the next sweep's strategy inf / inf = NaN, and a NaN reach below it
# is where the device and both CPU readings part (test_float_nan_reach_still_updates, below).

@pytest.mark.parametrize("dtype", ["f16", "f16+rmplus", "f32", "f32+rmplus"])
@pytest.mark.parametrize("fuse", [1, 0])
def test_float_edges_lanes(dtype, fuse):
    half = dtype.startswith("f16")
    for player in (0, 1):
        run_lanes(rs.default_flop(), [1], 1021, edge_float(half), float_utils(half), rmplus="rmplus" in dtype, dtype=dtype.split("+")[0],
                  scale=1.0, fuse=fuse, seed=41, iters=1, players=(player,))


@pytest.mark.parametrize("dtype", ["f16+rmplus", "f32"])
def test_float_edges_three_streets_enum(dtype):
    half = dtype.startswith("f16")
    for player in (0, 1):
        run_lanes(rs.three_street_options(), [1, 2, 6], 44, edge_float(half), float_utils(half), rmplus="rmplus" in dtype, dtype=dtype.split("+")[0],
                  chance="enum", scale=1.0, seed=42, iters=1, players=(player,))


@pytest.mark.xfail(strict=True, reason="known kernel issue: a NaN reach is the device's mark of an inactive lane, so a visit whose reach is NaN "
                                       "because an opponent's regrets reached +inf writes nothing, where cfr.rs's update (and both CPU readings) "
                                       "writes NaN, or 0 under RM+")
def test_float_nan_reach_still_updates():
    """two sweeps on binary16 rows near 65504: the first overflows regrets to +inf, the second reads sigma = inf / inf = NaN there"""
    run_lanes(rs.default_flop(), [1], 1021, edge_float(True), float_utils(True), dtype="f16", scale=1.0, seed=41, iters=1)


# ---- pair launches: both traversers of a chance-free lane tree in one kernel (rs_kernel_forms.pair_sweeps) ----------------------------------

SENTINEL = F32(-12345.678)   # what a root-utility buffer holds before an iteration: a null side's buffer must still hold it afterwards


def _of(x, player):
    return x[player] if isinstance(x, tuple) else x


def assert_no_nan_strategy(tab, what):
    """The input condition of the float pair cases: the reference forms no NaN strategy (inf / inf, its only source) that a later walk would read.  Where it does, the
    device's NaN-reach convention (test_float_nan_reach_still_updates) decides the outcome, not the pair kernel: such an input is to be changed, not skipped."""
    for idx, (R, _) in tab.items():
        with np.errstate(all="ignore"):
            bad = np.isnan(npr.get_strategy_f32(R)).any(axis=0)
        assert not bad.any(), "%s: node %d has a NaN strategy on %d lanes (first %d): change the test input" % (what, idx, int(bad.sum()), int(np.nonzero(bad)[0][0]))


def run_pair_lanes(options, boards, C, init, make_leaves, mode="clamp", prune=False, rmplus=False, dtype="i32", opp="full", seed=1, iters=3, scale=100.0,
                   graph=False, forms=None, nulls=None, settle=(), device=True):
    """run_lanes for a real pair launch.  Per iteration rs_iterate(h, 0, u0) and rs_iterate(h, 1, u1) with nothing in between, then the reads; the reference is
    iterate_lanes(player=0), iterate_lanes(player=1) with seeds sweep_seed(seed, 2 it), sweep_seed(seed, 2 it + 1).
    init, make_leaves: as for run_lanes, or a pair of them (player 0's nodes, player 1's / traverser 0's leaves, traverser 1's).  nulls: it -> (u0 is null, u1 is null).
    settle: the iterations in which a get_infosets between the two calls settles the held sweep (both sweeps of it then run plain; the seeds go on).
    device=False: the numpy side alone (the input condition of the float cases can be checked where there is no GPU)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_act, tree = rs.build_game_tree(options)
    nodes = npw.tree_from_records(tree.nodes)
    sampled = opp == "sample"
    tab = {}
    for nd in tree.action_nodes():
        R, S = _of(init, nd.player)(rng, nd.n_children, boards[nd.round_idx] * C)
        tab[nd.index] = (R.copy(), S.copy())
    ln = [{}, {}]
    for p in (0, 1):
        for i, d in enumerate(nodes):
            if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED":
                r = nodes[d["parent"]]["round_idx"]
                ln[p][i] = _of(make_leaves, p)(rng, r, boards[r] * C)
    if dtype != "i32":
        assert_no_nan_strategy(tab, "initial table")
    if device:
        table = rs.create_infosets(n_act, tree, [C], boards, DTYPES[dtype])
        for idx, (R, S) in tab.items():
            assert R.shape[1] == table.lanes(idx)
            table.upload_node(idx, R, S)
        lg = [{}, {}]
        for p in (0, 1):
            for i, (kind, buf) in ln[p].items():
                lg[p][i] = (rs.LEAF_UTIL if kind == "util" else rs.LEAF_SIGN, table.lane_buffer(nodes[nodes[i]["parent"]]["index"], 1, buf))
        m = (rs.UPD_WRAP_I32 if mode == "wrap" else rs.UPD_CLAMP_I64) | (rs.UPD_PRUNE if prune else 0) | (rs.UPD_RMPLUS if rmplus else 0)
        tr = rs.MCCFRTrainer(tree, table, lg[0], leaves_p1=lg[1], scale=scale, mode=m, chance_mode=rs.CHANCE_PASS, use_graph=graph, fuse_subtrees=1,
                             opp_mode=rs.OPP_SAMPLE if sampled else rs.OPP_FULL, sample_seed=seed, forms=forms)
        # a solver that fell back to plain sweeps must fail here, not pass below
        assert tr.paired, "the solver is not paired: these cases would compare plain sweeps"
        assert tr.n_launches(0) + tr.n_launches(1) == (2 if sampled else 1)
        root = tree.nodes[tree.nodes[0].children[0]].index
        u = [table.lane_buffer(root, 1), table.lane_buffer(root, 1)]   # allocated once: the same pointers every iteration (one captured graph per pair of pointers)
        sent = np.full(table.pitch(root), SENTINEL, dtype=F32)
        probe = next(nd.index for nd in tree.action_nodes() if nd.player == 0)
        lib = L.load()
    for it in range(iters):
        null = nulls(it) if nulls else (False, False)
        before = {i: (R.copy(), S.copy()) for i, (R, S) in tab.items()}
        if device:
            for b in u:
                b.upload(sent)
            L.check(lib.rs_iterate(tr._h, 0, None if null[0] else u[0].ptr))
            if it in settle:
                table.get_infosets(probe, np.arange(0, min(64, table.lanes(probe)), dtype=np.uint32))
            L.check(lib.rs_iterate(tr._h, 1, None if null[1] else u[1].ptr))
            got = [table.read_lane_buffer(b, root)[0] for b in u]
        want = []
        for player in (0, 1):
            want.append(npw.iterate_lanes(nodes, tab, ln[player], boards, C, player, scale=scale, mode=mode, prune=prune, rmplus=rmplus, dtype=dtype, chance="pass",
                                          opp=opp, seed=npr.sweep_seed(seed, 2 * it + player)))
            if dtype != "i32" and 2 * it + player < 2 * iters - 1:
                assert_no_nan_strategy(tab, "after sweep it=%d p=%d" % (it, player))
        if device:
            same_tables(table, tab, "pair it=%d" % it, before)
            for player in (0, 1):
                if null[player]:
                    assert_same(got[player], np.full(len(want[player]), SENTINEL, dtype=F32), "null root util buffer it=%d p=%d" % (it, player))
                else:
                    assert_same(got[player], want[player], "root util it=%d p=%d" % (it, player))
    if device:
        tr.destroy()
        table.destroy()
    return tab


def I32_UTILS(rng, r, n):   # drawn per traverser: the two walks' leaves differ
    return "util", edge_utils(rng, n)


@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+prune", "clamp+rmplus", "clamp+rmplus+prune"])
@pytest.mark.parametrize("graph,layout", [(False, "plain"), (True, "plain"), (False, "tiled64"), (True, "tiled64")])
def test_pair_i32_edges_river(mode, graph, layout, monkeypatch):
    """test_i32_edges_river through pair launches: 4 099 lanes, edge regrets, LEAF_UTIL leaves of each traverser's own, 3 iterations"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    run_pair_lanes(rs.default_flop(), [1], 4099, edge_i32, I32_UTILS, mode=mode.split("+")[0], prune="prune" in mode, rmplus="rmplus" in mode,
                   scale=10000.0 if mode == "wrap" else 100.0, graph=graph, seed=71)


def carry_f16(rng, A, n):
    """binary16 rows whose updates ROUND, in blocks of 16 lanes: (0) two positives 128 .. 2 176 below 65 504 (spacing 32; deltas below 16 a sweep: never 65 520, which would round to
    inf) and a large negative; (1) subnormal halves k * 2^-24; (2) rows x, x (sigma 1/2, 1/2: every product exact) with x an integer in [1 024, 2 048) (spacing 1) and even negatives
    in (-4 096, -2 048] (spacing 2), so that multiple-of-1/4 deltas land on round-to-nearest-even ties; (3) ordinary values with -0.0 and NaN cells"""
    blk = (np.arange(n) // 16) % 4
    R = npr.round_f16(rng.uniform(-1000, 1000, size=(A, n)))
    S = npr.round_f16(rng.uniform(0, 1000, size=(A, n)))
    R[:, blk == 0] = 65504.0 - 32.0 * rng.integers(4, 69, size=(A, int((blk == 0).sum())))
    R[A - 1, blk == 0] *= rng.choice([-1.0, 1.0], size=int((blk == 0).sum()))
    R[:, blk == 1] = rng.integers(-1023, 1024, size=(A, int((blk == 1).sum()))) * 2.0**-24
    x = rng.integers(1024, 2048, size=int((blk == 2).sum()))
    R[:, blk == 2] = -2.0 * rng.integers(1025, 2048, size=(A, int((blk == 2).sum())))
    R[0, blk == 2] = R[1, blk == 2] = x
    lanes3 = np.nonzero(blk == 3)[0]
    R[:, lanes3[::3]] = -0.0
    R[0, lanes3[1::5]] = np.nan
    assert (npr.round_f16(R)[~np.isnan(R)] == R[~np.isnan(R)]).all()
    return R.astype(F32), S.astype(F32)


def carry_f16_utils(rng, r, n):
    """utilities a few ulps of the row they meet: below 8 under 65 504, a few 2^-24 in the subnormal block, multiples of 1/2 in the tie block"""
    blk = (np.arange(n) // 16) % 4
    u = rng.uniform(-300, 300, size=n)
    u[blk == 0] = rng.uniform(-8, 8, size=int((blk == 0).sum()))
    u[blk == 1] = rng.integers(-6, 7, size=int((blk == 1).sum())) * 2.0**-24
    u[blk == 2] = rng.integers(-80, 81, size=int((blk == 2).sum())) * 0.5
    u = u.astype(F32)
    u[np.nonzero(blk == 3)[0][::7]] = F32(-0.0)
    return "util", u


def test_pair_f16_carry_rounding():
    """Row<F16>::carry: traverser 0's updated regrets stay in f32 registers and must come to the second walk as binary16 would give them back.  Every update of three blocks
    in four rounds (ties, subnormals, spacing 32 below 65 504); 3 iterations, so that traverser 1's sigma of iteration 1 and everything after depend on it.  No value overflows."""
    tab = run_pair_lanes(rs.default_flop(), [1], 1021, carry_f16, carry_f16_utils, dtype="f16", scale=1.0, seed=73, iters=3)
    assert all(np.isfinite(R[~np.isnan(R)]).all() for R, _ in tab.values())


# The NaN-reach rule (test_float_nan_reach_still_updates): a pair cannot take one sweep per fresh table, so the inputs keep what overflows where no later walk reads it -- rows
# near the largest finite value on player 1's nodes, overflowing utilities on traverser 1's leaves, one iteration (traverser 1's is the last sweep) -- and NaN cells, NaN
# utilities, -0.0 and subnormal halves everywhere.  run_pair_lanes asserts the condition on the reference (assert_no_nan_strategy).  The inputs that do overflow on player 0's
# nodes are compared pair ON against pair OFF instead (tests/test_gpu_pair_sweeps.py).
@pytest.mark.parametrize("dtype", ["f16", "f16+rmplus", "f32", "f32+rmplus"])
def test_pair_float_edges_lanes(dtype):
    half = dtype.startswith("f16")
    run_pair_lanes(rs.default_flop(), [1], 1021, (edge_float(half, big_rows=False), edge_float(half)), (float_utils(half, big=False), float_utils(half)),
                   rmplus="rmplus" in dtype, dtype=dtype.split("+")[0], scale=1.0, seed=75, iters=1)


@pytest.mark.parametrize("lanes_per_thread", ["1", "2", "4"])
@pytest.mark.parametrize("C", [4099, 37])
@pytest.mark.parametrize("case", ["i32-clamp+prune", "f16-carry"])
def test_pair_lanes_per_thread(case, C, lanes_per_thread, monkeypatch):
    """the pair kernel's three forms (RS_JIT_LANES; its own default is 2) over 64-lane table tiles: a tile shift and a vector count rescaled from the four-lane kernels' arguments, at
    lane counts that are no multiple of 4 or 64 and below one tile"""
    monkeypatch.setenv("RS_JIT_LANES", lanes_per_thread)
    monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    if case == "f16-carry":
        run_pair_lanes(rs.default_flop(), [1], C, carry_f16, carry_f16_utils, dtype="f16", scale=1.0, seed=77, iters=2)
    else:
        run_pair_lanes(rs.default_flop(), [1], C, edge_i32, I32_UTILS, prune=True, seed=79, iters=2)


@pytest.mark.parametrize("settle", [(), (1,)], ids=["pairs", "settled-between"])
def test_pair_i32_edges_river_sampled(settle):
    """OPP_SAMPLE with prune, 3 boards x 1 367 clusters: the two seeds of an iteration come from one k_next_seed_pair launch and must be sweep_seed(seed, 2 it) and (seed, 2 it + 1) --
    also when iteration 1's held sweep was settled as a plain one (two k_next_seed launches) between two pair launches"""
    run_pair_lanes(rs.default_flop(), [3], 1367, edge_i32, I32_UTILS, prune=True, opp="sample", seed=81, iters=4 if settle else 3, settle=settle)


@pytest.mark.parametrize("graph", [True, False])
def test_pair_null_root_utilities(graph):
    """either root-utility pointer may be null: tables and the other side's output are what they are otherwise, the null side's buffer is not written, and under graph replay
    every pair of pointers gets its own graph (7 iterations: both, u0 null, u1 null, both null, then the first three pairs again)"""
    pattern = [(False, False), (True, False), (False, True), (True, True), (False, False), (True, False), (False, True)]
    run_pair_lanes(rs.default_flop(), [1], 4099, edge_i32, I32_UTILS, rmplus=True, graph=graph, seed=83, iters=len(pattern), nulls=lambda it: pattern[it])


# ---- deal sweeps -------------------------------------------------------------------------------------------------------------

def run_deals(options, sizes, n_deals, seed, init, util_mag=None, mode="clamp", prune=False, per_deal=False, rmplus=False, dtype="i32",
              opp="sample", scale=100.0, iters=2, fuse=1, graph=False, check=None, players=(0, 1)):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_act, tree = rs.build_game_tree(options)
    nodes = npw.tree_from_records(tree.nodes)
    table = rs.create_infosets(n_act, tree, sizes, [1] * len(sizes), DTYPES[dtype])
    tab = {}
    for nd in tree.action_nodes():
        R, S = init(rng, nd.n_children, sizes[nd.round_idx][nd.player])
        table.upload_node(nd.index, R, S)
        tab[nd.index] = (R.copy(), S.copy())
    cidx = {(r, p): rng.integers(0, sizes[r][p], size=n_deals).astype(np.uint32) for r in range(len(sizes)) for p in (0, 1)}
    if util_mag is None:
        buf, kind = rng.integers(-1, 2, size=n_deals).astype(F32), "sign"
    else:
        buf, kind = (rng.uniform(-1, 1, size=n_deals) * util_mag).astype(F32), "util"
    dbuf = rs.deal_buffer(table, n_deals, buf)
    term = [i for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"]
    lg = {i: (rs.LEAF_UTIL if kind == "util" else rs.LEAF_SIGN, dbuf) for i in term}
    ln = {i: (kind, buf) for i in term}
    flags = (rng.integers(0, 3, n_deals) == 0).astype(np.uint8) if per_deal else None
    m = (rs.UPD_WRAP_I32 if mode == "wrap" else rs.UPD_CLAMP_I64) | (rs.UPD_PRUNE if prune else 0) | (rs.UPD_RMPLUS if rmplus else 0)
    tr = rs.MCCFRTrainer(tree, table, lg, scale=scale, mode=m, fuse_subtrees=fuse, deals=cidx, opp_mode=rs.OPP_SAMPLE if opp == "sample" else rs.OPP_FULL,
                         sample_seed=seed, use_graph=graph, prune_deal=flags)
    if check:
        check(tr)
    k = 0
    for it in range(iters):
        for player in players:
            got = tr.iterate(player, want_root_util=True)
            want = npw.iterate_deals(nodes, tab, ln, cidx, player, scale=scale, mode=mode, prune=prune, prune_deal=flags, rmplus=rmplus, dtype=dtype,
                                     opp=opp, seed=npr.sweep_seed(seed, k))
            k += 1
            assert_same(got, want, "root util it=%d p=%d" % (it, player))
    same_tables(table, tab)


DEAL_FORMS = {
    "auto": {},
    "lanes2": {"RS_JIT_LANES": "2"},
    "lanes4": {"RS_JIT_LANES": "4"},
    "no-merge": {"RS_JIT_NO_MERGE": "1"},
    "rows": {"RS_JIT_ROWS": "1", "RS_JIT_SCAN_ALL": "0"},
    "ordered": {"RS_JIT_ORDERED": "1", "RS_JIT_ROWS": "0"},
    "rows+ordered": {"RS_JIT_ROWS": "1", "RS_JIT_ORDERED": "1", "RS_JIT_SCAN_ALL": "0"},
    "scan-all": {"RS_JIT_SCAN_ALL": "1", "RS_JIT_ROWS": "0", "RS_JIT_ORDERED": "0"},
    "lds-max": {"RS_JIT_LDS_MAX": "8256", "RS_JIT_ROWS": "0", "RS_JIT_ORDERED": "0"},
}


@pytest.mark.parametrize("form", sorted(DEAL_FORMS))
@pytest.mark.parametrize("variant", ["river-prune-per-deal", "three-streets"])
def test_i32_edge_deal_forms(form, variant, monkeypatch):
    """about 1 000 deals on 13 / 17 clusters (three streets: 3 000 deals), edge regrets, LEAF_UTIL deltas up to 4e9, through every deal form"""
    for k, v in DEAL_FORMS[form].items():
        monkeypatch.setenv(k, v)
    if variant.startswith("river"):
        run_deals(rs.default_flop(), [(13, 17)], 1000, 51, edge_i32, util_mag=2e7, prune=True, per_deal=True)
    else:
        sizes = [(7, 9), (211, 190), (301, 250)] if form == "lds-max" else [(7, 9), (11, 8), (13, 17)]
        run_deals(rs.three_street_options(), sizes, 3000, 52, edge_i32, util_mag=4e7, prune=True)


def _assert_delta_rows(tr):
    assert tr.delta_rows


def test_i32_direct_rows_beyond_16384_clusters(monkeypatch):
    """a round of 17 000 / 16 500 clusters: its deltas go straight into the table (direct rows)"""
    monkeypatch.setenv("RS_JIT_ROWS", "1")
    run_deals(rs.three_street_options(), [(7, 9), (11, 8), (17000, 16500)], 20011, 53, edge_i32, util_mag=2e7, prune=True, per_deal=True,
              check=_assert_delta_rows)


@pytest.mark.parametrize("dtype", ["f16", "f16+rmplus", "f32+rmplus"])
@pytest.mark.parametrize("variant", ["river", "three-streets-full", "river-direct"])
def test_float_edge_deals(dtype, variant, monkeypatch):
    half = dtype.startswith("f16")
    dt, rmplus = dtype.split("+")[0], "rmplus" in dtype
    mag = 3e4 if half else 1e37
    for player in (0, 1):   # one sweep per fresh table, as for the lane sweeps above
        if variant == "river":
            run_deals(rs.default_flop(), [(13, 17)], 1500, 61, edge_float(half), util_mag=mag, rmplus=rmplus, dtype=dt, scale=1.0, iters=1, players=(player,))
        elif variant == "river-direct":
            run_deals(rs.default_flop(), [(16500, 17000)], 20011, 62, edge_float(half), util_mag=mag, rmplus=rmplus, dtype=dt, scale=1.0, iters=1,
                      players=(player,))
        else:
            run_deals(rs.three_street_options(), [(7, 9), (11, 8), (13, 17)], 400, 63, edge_float(half), util_mag=mag, rmplus=rmplus, dtype=dt,
                      opp="full", scale=1.0, iters=1, players=(player,))


# ---- DealTrainer batches replayed deal for deal ----------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["f16+rmplus", "i32+prune"])
def test_deal_trainer_batches_replayed(variant):
    """rs_deal_trainer: after every batch the live cluster ids, signs and prune flags are read back and the batch is replayed through
    np_walk.iterate_deals (both traversers, then the discount check); the tables must stay bit-equal"""
    half = variant.startswith("f16")
    mask = ab.card_mask("4d5dAs3cKs")
    hands = ab.random_range(mask)
    n_deals, seed, interval = 2000, 17, 5000
    n_act, tree = rs.build_game_tree(rs.default_flop())
    nodes = npw.tree_from_records(tree.nodes)
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, 2, None)]
    dt = "f16" if half else "i32"
    tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, n_deals, seed=seed, discount_interval=interval, discount_cap=10**9,
                        prune_threshold=None if half else 3000, scale=0.5 if half else 100.0, dtype=DTYPES[dt],
                        mode=rs.UPD_CLAMP_I64 | (rs.UPD_RMPLUS if half else 0))
    sizes = [(a.get_size(0), a.get_size(1)) for a in card_abs]
    rng = np.random.Generator(np.random.PCG64(5))
    tab = {}
    for nd in tree.action_nodes():
        if half:
            R, S = edge_float(True, big_rows=False)(rng, nd.n_children, sizes[0][nd.player])   # no +inf regrets: see test_float_nan_reach_still_updates
        else:
            R, S = edge_i32(rng, nd.n_children, sizes[0][nd.player])
        tr.infosets.upload_node(nd.index, R, S)
        tab[nd.index] = (R.copy(), S.copy())
    term = [i for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"]
    t, threshold, k, pruned = 0, interval, 0, 0
    for b in range(4):
        tr.train(1)
        cidx = {(0, p): tr.clusters(0, p) for p in (0, 1)}
        leaves = {i: ("sign", tr.signs()) for i in term}
        flags = None if half else tr.prune_flags()
        pruned += 0 if flags is None else int(flags.sum())
        for player in (0, 1):
            npw.iterate_deals(nodes, tab, leaves, cidx, player, scale=0.5 if half else 100.0, mode="clamp", prune=not half, prune_deal=flags,
                              rmplus=half, dtype=dt, opp="sample", seed=npr.sweep_seed(seed, k))
            k += 1
        t += n_deals
        if t > threshold:
            npw.discount_table(tab, npr.discount_factor(t, interval), dt)
            threshold = t + interval
        same_tables(tr.infosets, tab, "batch %d" % b)
    assert half or pruned > 0
