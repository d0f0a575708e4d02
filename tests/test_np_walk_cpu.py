"""CPU: the numpy restatement of the whole tree walks (oracle/np_walk.py, written from cfr.rs) against the C oracle (rs_oracle.c),
bit for bit: root utilities and whole tables, both traversers, several sweeps, over the lane model (river, three streets, random option
trees; ENUM and PASS chance; FULL and sampled opponents; clamp / wrap / prune; RM+, f32, binary16; LEAF_UTIL leaves), deal batches with
heavy collisions, and the train() schedule with discount ticks.  Two independent readings of the reference that agree here leave the
kernels, which are checked against either, less room to share a misreading."""
import numpy as np
import pytest

from oracle import np_restate as npr
from oracle import np_walk as npw
from oracle import orc

F32 = np.float32
THREE = dict(n_board_cards=3, bet_sizes=((0.5, 1.0),) * 3, raise_sizes=((3.0,),) * 3)   # orc_options_three_street
RIVER = dict(n_board_cards=5, bet_sizes=((0.5, 1.0),), raise_sizes=((3.0,),))           # options::default_flop()
DT = {"i32": orc.T_I32, "f32": orc.T_F32, "f16": orc.T_F16}


def canon(x):
    """f32 bit patterns with every NaN made one (x86 and numpy do not agree on the sign of a NaN that inf - inf makes)"""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def assert_same(got, want, what):
    if np.asarray(want).dtype == np.int32:
        bad = np.nonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))[0]
    else:
        bad = np.nonzero(canon(got) != canon(want))[0]
    assert bad.size == 0, "%s: %d values differ, first at %d: %r vs %r" % (what, bad.size, bad[0], np.asarray(got).reshape(-1)[bad[0]],
                                                                        np.asarray(want).reshape(-1)[bad[0]])


def trees(opts):
    """the same public tree twice: np_restate.build_tree's dicts and the C oracle's, with the node numbering checked to agree"""
    o = dict(stacks=(500, 500), pot=35, **opts)
    nodes, n_act = npr.build_tree(o["stacks"], o["pot"], o["n_board_cards"], o["bet_sizes"], o["raise_sizes"])
    otree = orc.OracleTree(orc.make_options(o["stacks"], o["pot"], o["n_board_cards"], o["bet_sizes"], o["raise_sizes"]))
    kinds = {npw.PRIVATE: orc.PRIVATE_CHANCE, npw.PUBLIC: orc.PUBLIC_CHANCE, npw.ACTION: orc.ACTION, npw.TERMINAL: orc.TERMINAL}
    od = otree.as_dicts()
    assert n_act == otree.n_action_nodes and len(nodes) == len(od)
    for a, b in zip(nodes, od):
        assert kinds[a["kind"]] == b["kind"] and a["children"] == b["children"]
        if a["kind"] == npw.ACTION:
            assert (a["index"], a["player"], a["round_idx"]) == (b["index"], b["player"], b["round_idx"])
        if a["kind"] == npw.TERMINAL:
            assert (a["value"], a["last_to_act"]) == (b["value"], b["last_to_act"])
            assert a["ttype"] == {orc.ALLIN: "ALLIN", orc.SHOWDOWN: "SHOWDOWN", orc.UNCONTESTED: "UNCONTESTED"}[b["ttype"]]
    return nodes, otree


def fill(rng, nodes, width, dtype, regret_scale=10**6):
    """random table {index: (R, S)}; width(node dict) -> lanes of that node's row.  i32 rows carry prune and saturation lanes."""
    tab = {}
    for d in nodes:
        if d["kind"] != npw.ACTION:
            continue
        a, n = len(d["children"]), width(d)
        if dtype == "i32":
            R = rng.integers(-regret_scale, regret_scale, size=(a, n)).astype(np.int32)
            S = rng.integers(0, regret_scale, size=(a, n)).astype(np.int32)
            if a > 0:
                R[0, ::11] = -10_000_001
                R[0, 5::11] = -10_000_000          # the threshold itself is pruned (cfr.rs:380 is a strict >)
                R[a - 1, ::13] = 2_147_000_000
        else:
            R = rng.uniform(-1000, 1000, size=(a, n)).astype(F32)
            S = rng.uniform(0, 1000, size=(a, n)).astype(F32)
            if dtype == "f16":
                R, S = npr.round_f16(R), npr.round_f16(S)
        tab[d["index"]] = (R, S)
    return tab


def load(otab, tab):
    for idx, (R, S) in tab.items():
        otab.set_node(idx, R, S)


def same_tables(otab, tab, what=""):
    for idx, (R, S) in tab.items():
        ro, so = otab.get_node(idx)
        assert_same(R, ro, "%s regrets of node %d" % (what, idx))
        assert_same(S, so, "%s strategy sums of node %d" % (what, idx))


def lane_leaves(rng, nodes, n_boards, C, kind="sign"):
    """one sign vector per round (its lanes), or one utility vector per terminal"""
    np_leaves, o_leaves, signs = {}, {}, {}
    for i, d in enumerate(nodes):
        if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED":
            r = nodes[d["parent"]]["round_idx"]
            if kind == "sign":
                if r not in signs:
                    signs[r] = rng.integers(-1, 2, size=n_boards[r] * C).astype(F32)
                buf = signs[r]
            else:
                buf = rng.uniform(-3000, 3000, size=n_boards[r] * C).astype(F32)
            np_leaves[i] = (kind, buf)
            o_leaves[i] = (orc.LEAF_SIGN if kind == "sign" else orc.LEAF_UTIL, buf)
    return np_leaves, o_leaves


def run_lanes(opts, boards, C, seed, chance="enum", opp="full", mode="wrap", prune=False, rmplus=False, dtype="i32", iters=3, leaf="sign",
              regret_scale=10**6, scale=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes, otree = trees(opts)
    tab = fill(rng, nodes, lambda d: boards[d["round_idx"]] * C, dtype, regret_scale)
    otab = orc.OracleTable(otree, boards, C, DT[dtype])
    load(otab, tab)
    npl, ol = lane_leaves(rng, nodes, boards, C, leaf)
    if scale is None:
        scale = 10000.0 if mode == "wrap" else (100.0 if dtype == "i32" else 0.5)
    osol = orc.OracleSolver(otree, otab, ol, scale=scale, mode=orc.UPD_WRAP_I32 if mode == "wrap" else orc.UPD_CLAMP_I64, prune=prune,
                            rmplus=rmplus, chance_mode=orc.CHANCE_ENUM if chance == "enum" else orc.CHANCE_PASS,
                            opp_mode=orc.OPP_SAMPLE if opp == "sample" else orc.OPP_FULL, base_seed=seed)
    for it in range(iters):
        for player in (0, 1):
            s = npr.sweep_seed(seed, osol.calls)
            want = osol.iterate(player)
            got = npw.iterate_lanes(nodes, tab, npl, boards, C, player, scale=scale, mode=mode, prune=prune, rmplus=rmplus, dtype=dtype,
                                    chance=chance, opp=opp, seed=s)
            assert_same(got, want, "root util it=%d p=%d" % (it, player))
    same_tables(otab, tab)
    return nodes, tab


# ---- lane sweeps --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+prune"])
@pytest.mark.parametrize("opp", ["full", "sample"])
@pytest.mark.parametrize("C,B", [(5, 1), (37, 3)])
def test_river_lanes(mode, opp, C, B):
    run_lanes(RIVER, [B], C, C + B, chance="pass", opp=opp, mode=mode.split("+")[0], prune="prune" in mode)


@pytest.mark.parametrize("boards,chance", [([1, 2, 6], "enum"), ([1, 1, 1], "enum"), ([1, 3, 3], "enum"), ([2, 2, 2], "pass")])
@pytest.mark.parametrize("mode", ["clamp", "wrap", "clamp+prune"])
def test_three_street_lanes(boards, chance, mode):
    run_lanes(THREE, boards, 7, 40 + boards[-1], chance=chance, mode=mode.split("+")[0], prune="prune" in mode, iters=3)


@pytest.mark.parametrize("mode", ["clamp", "clamp+prune"])
def test_three_street_sampled_lanes(mode):
    run_lanes(THREE, [3, 3, 3], 5, 47, chance="pass", opp="sample", mode="clamp", prune="prune" in mode)


@pytest.mark.parametrize("dtype", ["i32+rmplus", "f32", "f16", "f32+rmplus", "f16+rmplus"])
@pytest.mark.parametrize("shape", ["river-full", "river-sample", "three-enum"])
def test_extension_dtypes_lanes(dtype, shape):
    dt, rmplus = dtype.split("+")[0], "rmplus" in dtype
    if shape == "three-enum":
        run_lanes(THREE, [1, 2, 6], 6, 61, chance="enum", mode="clamp", rmplus=rmplus, dtype=dt)
    else:
        run_lanes(RIVER, [2], 50, 62, chance="pass", opp=shape.split("-")[1], mode="clamp", rmplus=rmplus, dtype=dt)


def test_i32_rmplus_with_prune_lanes():
    """RM+ with pruning (both are allowed together on i32 tables): the regrets below the threshold are pruned like cfr.rs:379-386"""
    run_lanes(THREE, [1, 3, 3], 5, 63, chance="enum", mode="clamp", prune=True, rmplus=True)


@pytest.mark.parametrize("shape", ["river", "three-enum"])
def test_leaf_util_lanes(shape):
    """LEAF_UTIL leaves: utilities given verbatim, one buffer per terminal, with deltas far beyond 2^31 (clamp) and wrapping (wrap)"""
    if shape == "river":
        run_lanes(RIVER, [2], 33, 12, chance="pass", mode="clamp", leaf="util", scale=1e6)
        run_lanes(RIVER, [2], 33, 13, chance="pass", mode="wrap", leaf="util", scale=1e6)
    else:
        run_lanes(THREE, [1, 2, 6], 4, 14, chance="enum", mode="clamp", prune=True, leaf="util", scale=1e5)


@pytest.mark.parametrize("seed", range(12))
def test_random_option_trees_lanes(seed):
    """the random option trees of test_random_options_trees_match_oracle, with a random board fan, mode and opponent"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nb = int(rng.integers(3, 6))
    rounds = 6 - nb
    bets = [sorted(rng.choice([0.25, 0.33, 0.5, 0.75, 1.0, 1.5, 2.0], size=int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(rounds)]
    raises = [sorted(rng.choice([2.0, 2.5, 3.0, 4.0], size=int(rng.integers(1, 3)), replace=False).tolist()) for _ in range(rounds)]
    stacks = (int(rng.integers(20, 2000)), int(rng.integers(20, 2000)))
    pot = int(rng.integers(2, 300))
    nodes, n_act = npr.build_tree(stacks, pot, nb, bets, raises)
    otree = orc.OracleTree(orc.make_options(stacks, pot, nb, bets, raises))
    assert n_act == otree.n_action_nodes and [d["children"] for d in nodes] == [d["children"] for d in otree.as_dicts()]
    boards = [1]
    for _ in range(1, rounds):
        boards.append(boards[-1] * int(rng.integers(1, 4)))
    C = int(rng.integers(2, 9))
    sampled = bool(rng.integers(0, 2)) and all(len(d["children"]) > 0 for d in nodes if d["kind"] == npw.ACTION)
    chance = "pass" if sampled else "enum"
    if chance == "pass":
        boards = [boards[-1]] * rounds
    mode = ["clamp", "wrap"][int(rng.integers(0, 2))]
    prune = mode == "clamp" and bool(rng.integers(0, 2))
    tab = fill(rng, nodes, lambda d: boards[d["round_idx"]] * C, "i32")
    otab = orc.OracleTable(otree, boards, C)
    load(otab, tab)
    npl, ol = lane_leaves(rng, nodes, boards, C)
    scale = 10000.0 if mode == "wrap" else 100.0
    osol = orc.OracleSolver(otree, otab, ol, scale=scale, mode=orc.UPD_WRAP_I32 if mode == "wrap" else orc.UPD_CLAMP_I64, prune=prune,
                            chance_mode=orc.CHANCE_ENUM if chance == "enum" else orc.CHANCE_PASS,
                            opp_mode=orc.OPP_SAMPLE if sampled else orc.OPP_FULL, base_seed=seed)
    for it in range(3):
        for player in (0, 1):
            s = npr.sweep_seed(seed, osol.calls)
            want = osol.iterate(player)
            got = npw.iterate_lanes(nodes, tab, npl, boards, C, player, scale=scale, mode=mode, prune=prune, chance=chance,
                                    opp="sample" if sampled else "full", seed=s)
            assert_same(got, want, "root util it=%d p=%d" % (it, player))
    same_tables(otab, tab)


def test_train_with_discount_ticks():
    """train()'s schedule (cfr.rs:188-265) with interval 3 and cap 9: ticks after t = 4 and t = 8, none past the cap"""
    rng = np.random.Generator(np.random.PCG64(3))
    nodes, otree = trees(RIVER)
    C = 24
    tab = fill(rng, nodes, lambda d: C, "i32")
    otab = orc.OracleTable(otree, [1], C)
    load(otab, tab)
    npl, ol = lane_leaves(rng, nodes, [1], C)
    osol = orc.OracleSolver(otree, otab, ol, scale=100.0, mode=orc.UPD_CLAMP_I64, chance_mode=orc.CHANCE_PASS)
    osol.train(11, discount_interval=3, discount_cap=9)
    seen = []
    orig = npw.discount_table
    npw.discount_table = lambda t, d, dt="i32": (seen.append(float(d)), orig(t, d, dt))
    try:
        npw.train_lanes(nodes, tab, npl, [1], C, 11, discount_interval=3, discount_cap=9, scale=100.0, mode="clamp", chance="pass")
    finally:
        npw.discount_table = orig
    assert seen == [0.5, 2.0 / 3.0] or seen == [float(npr.discount_factor(4, 3)), float(npr.discount_factor(8, 3))]
    same_tables(otab, tab)


# ---- deal sweeps -----------------------------------------------------------------------------------------------------------

def deal_setup(opts, sizes, n_deals, seed, dtype="i32", leaf="sign"):
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes, otree = trees(opts)
    tab = fill(rng, nodes, lambda d: sizes[d["round_idx"]][d["player"]], dtype)
    otab = orc.OracleDealTable(otree, sizes, DT[dtype])
    load(otab, tab)
    cidx = {(r, p): rng.integers(0, sizes[r][p], size=n_deals).astype(np.uint32) for r in range(len(sizes)) for p in (0, 1)}
    if leaf == "sign":
        sign = rng.integers(-1, 2, size=n_deals).astype(F32)
        npl = {i: ("sign", sign) for i, d in enumerate(nodes) if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"}
    else:
        npl = {i: ("util", rng.uniform(-2000, 2000, size=n_deals).astype(F32)) for i, d in enumerate(nodes)
               if d["kind"] == npw.TERMINAL and d["ttype"] != "UNCONTESTED"}
    ol = {i: (orc.LEAF_SIGN if k == "sign" else orc.LEAF_UTIL, b) for i, (k, b) in npl.items()}
    return rng, nodes, otree, tab, otab, cidx, npl, ol


def run_deals(opts, sizes, n_deals, seed, mode="clamp", prune=False, per_deal=False, rmplus=False, dtype="i32", opp="sample", lane_base=0,
              leaf="sign", scale=None):
    rng, nodes, otree, tab, otab, cidx, npl, ol = deal_setup(opts, sizes, n_deals, seed, dtype, leaf)
    flags = (rng.integers(0, 3, n_deals) == 0).astype(np.uint8) if per_deal else None
    if scale is None:
        scale = 10000.0 if mode == "wrap" else (100.0 if dtype == "i32" else 0.25)
    osol = orc.OracleDealSolver(otree, otab, ol, cidx, n_deals, lane_base=lane_base, prune_deal=flags, scale=scale,
                                mode=orc.UPD_WRAP_I32 if mode == "wrap" else orc.UPD_CLAMP_I64, prune=prune, rmplus=rmplus,
                                opp_mode=orc.OPP_SAMPLE if opp == "sample" else orc.OPP_FULL, base_seed=seed)
    for it in range(3):
        for player in (0, 1):
            s = npr.sweep_seed(seed, osol.calls)
            want = osol.iterate(player)
            got = npw.iterate_deals(nodes, tab, npl, cidx, player, scale=scale, mode=mode, prune=prune, prune_deal=flags, rmplus=rmplus,
                                    dtype=dtype, opp=opp, seed=s, lane_base=lane_base)
            assert_same(got, want, "root util it=%d p=%d" % (it, player))
    same_tables(otab, tab)


@pytest.mark.parametrize("variant", ["clamp", "wrap", "clamp+prune", "clamp+prune-per-deal", "full", "full+prune-per-deal", "lane-base",
                                     "rmplus", "rmplus+prune-per-deal", "leaf-util"])
def test_river_deals(variant):
    """about 1 000 deals on 13 / 17 clusters: 60-80 deals per info set"""
    run_deals(RIVER, [(13, 17)], 1000, 70, mode="wrap" if variant == "wrap" else "clamp", prune="prune" in variant,
              per_deal="per-deal" in variant, rmplus="rmplus" in variant, opp="full" if variant.startswith("full") else "sample",
              lane_base=123_456_789 if variant == "lane-base" else 0, leaf="util" if variant == "leaf-util" else "sign")


@pytest.mark.parametrize("variant", ["sample", "full", "sample+prune-per-deal", "wrap", "lane-base"])
def test_three_street_deals(variant):
    run_deals(THREE, [(7, 9), (11, 8), (13, 17)], 300, 71, mode="wrap" if variant == "wrap" else "clamp", prune="prune" in variant,
              per_deal="per-deal" in variant, opp="full" if variant == "full" else "sample", lane_base=5_000_000_003 if variant == "lane-base" else 0)


@pytest.mark.parametrize("dtype", ["f32", "f16", "f32+rmplus", "f16+rmplus"])
@pytest.mark.parametrize("shape", ["river-sample", "river-full", "three-sample"])
def test_float_deals(dtype, shape):
    """f32 deltas summed from 0.0 in deal order, one rounding per cell on the write-back, the RM+ floor there, the traverser's rows only"""
    dt, rmplus = dtype.split("+")[0], "rmplus" in dtype
    if shape.startswith("three"):
        run_deals(THREE, [(7, 9), (11, 8), (13, 17)], 500, 72, dtype=dt, rmplus=rmplus, opp="sample", lane_base=77)
    else:
        run_deals(RIVER, [(13, 17)], 1000, 73, dtype=dt, rmplus=rmplus, opp=shape.split("-")[1])


def test_deal_order_sums_are_sequential():
    """the per-cell sums add in deal order: a big value then its negation then a small one gives the small one, not 0"""
    cells = np.array([1, 0, 1, 1, 0], dtype=np.int64)
    d = np.array([1e8, 1.0, -1e8, 3.0, 2.0], dtype=F32)
    out = npw._deal_order_sums(cells, d, 3)
    assert out.tolist() == [3.0, 3.0, 0.0]
    d2 = np.array([3.0, 1.0, 1e8, -1e8, 2.0], dtype=F32)
    assert npw._deal_order_sums(cells, d2, 3).tolist() == [3.0, 0.0, 0.0]   # (3 + 1e8) rounds to 1e8, then - 1e8
