"""GPU (-m gpu): the device's lane and deal sweeps against the numpy restatement of the walks (oracle/np_walk.py), with no C oracle in
between, at the numeric edges where kernels go wrong: i32 regrets at INT32_MIN / INT32_MAX and around the prune threshold, LEAF_UTIL deltas
that straddle 2^31 and 2^32 in waves that are all small, all large or mixed (the wave-uniform fast path of visit_i32), NaN and +-inf
utilities, zero-probability opponent actions, all-non-positive rows; binary16 rows that overflow to inf, subnormal halves, -0.0 and NaN
reaching the RM+ floor, f32 near FLT_MAX; lane counts that are no multiple of 4 or 64, fused and level plans, both lane-fan forms, graph
replay, 64-lane table tiles, the deal-sweep forms, a round beyond 16 384 clusters, and DealTrainer batches replayed deal for deal.
Bar: bit-equal, every NaN counted as one value."""
import numpy as np
import pytest

import rustsolver_amd as rs
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


# ---- i32 tables through whole walks --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+prune", "clamp+rmplus", "clamp+rmplus+prune"])
@pytest.mark.parametrize("fuse,graph,layout", [(1, False, "plain"), (0, False, "plain"), (1, True, "tiled64"), (0, True, "tiled64")])
def test_i32_edges_river(mode, fuse, graph, layout, monkeypatch):
    """the river tree over 4 099 lanes (no multiple of 4 or 64) with edge regrets and LEAF_UTIL leaves whose deltas straddle 2^31 and 2^32"""
    if layout == "tiled64":
        monkeypatch.setenv("RS_TABLE_TILE_LANES", "64")
    run_lanes(rs.default_flop(), [1], 4099, edge_i32, lambda rng, r, n: ("util", edge_utils(rng, n)), mode=mode.split("+")[0], prune="prune" in mode,
              rmplus="rmplus" in mode, scale=10000.0 if mode == "wrap" else 100.0, fuse=fuse, graph=graph, seed=11 + fuse)


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


def float_utils(half):
    def make(rng, r, n):
        blk = (np.arange(n) // 16) % 4
        u = rng.uniform(-500, 500, size=n).astype(F32)
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
