"""GPU (-m gpu): deal sweeps on float tables (binary32 and binary16, optionally RM+) whose rounds have more than 16 384 clusters.  The apply sums every cell's per-deal
f32 deltas in deal order; its member lists come from the radix sort above 16 384 clusters (the counting sort's LDS histogram ends there).  The flop-start game with the
reference's lossless (ISOMORPHIC) river has tens of thousands of river clusters: same bits as the oracle chain, batch after batch."""
import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import orc
from rustsolver_amd import abstraction as ab
from tests.test_gpu_cards import compare_trainer_tables, load_trainer_pair, oracle_batch

pytestmark = pytest.mark.gpu

LDS_MAX_CLUSTERS = 16384


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need a real MI355X (there is no CPU fallback)")


def assert_bits(a, b, what):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel()
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.uint32).ravel()
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d/%d values differ, first at %d: %08x vs %08x" % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]])


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_deal_trainer_float_tables_isomorphic_river(dtype):
    """the three-street game from a flop with bucket files on flop and turn and the ISOMORPHIC river (cfr.rs:159-184): 40 / 55 hole-card combos give each player
    more than 16 384 river clusters.  A binary16 (or f32) table trains it across a discount tick, bit-equal to the oracle chain; pruning stays refused."""
    rng = np.random.Generator(np.random.PCG64(79))
    mask = ab.card_mask("7h8hQc")
    allh = ab.random_range(mask)
    ranges = [allh[rng.permutation(len(allh))[:40]], allh[rng.permutation(len(allh))[:55]]]
    files = [rng.integers(0, 37, size=1286792, dtype=np.uint32), rng.integers(0, 61, size=13960050, dtype=np.uint32), None]
    dt_g, dt_o = (rs.F16, orc.T_F16) if dtype == "f16" else (rs.F32, orc.T_F32)
    ctx = load_trainer_pair(rs.three_street_options(), orc.options_three_street(), mask, ranges, 3, 1200, seed=8, interval=2000, cap=10**9, bucket_files=files, odtype=dt_o,
                            scale=0.5, dtype=dt_g)
    river = [ctx["card_abs"][2].get_size(p) for p in (0, 1)]
    print("ISOMORPHIC river clusters per player: %s" % river)
    assert min(river) > LDS_MAX_CLUSTERS, river
    for b in range(4):
        ctx["tr"].train(1 if b else 2)
        cards = oracle_batch(ctx)
        if not b:
            cards = oracle_batch(ctx)
        assert (ctx["tr"].cards() == cards).all()
    ctx["tr"].status()
    assert ctx["tr"].iterations == 5 * 1200 == ctx["t"]
    compare_trainer_tables(ctx)
    n_actions, tree = rs.build_game_tree(rs.three_street_options())
    with pytest.raises(rs.RsError):   # cfr.rs:352 compares i32 regrets
        rs.DealTrainer(tree, ctx["card_abs"], ranges, mask, 64, dtype=dt_g, prune_threshold=10**7)


@pytest.mark.parametrize("variant", ["river", "three-street"])
@pytest.mark.parametrize("dtype", ["f32+rmplus", "f16+rmplus"])
def test_float_deal_batches_rmplus_large_rounds(variant, dtype):
    """rs_solver_create_deals on a float table with RM+ and a last round of 20 000 - 30 000 clusters against a few thousand deals: most cells see no deal, and the
    apply still touches every one of them (one rounding, the RM+ clamp, -0 to +0) exactly as the oracle's sequential loop does.  Root utilities too."""
    three = variant == "three-street"
    half = dtype.startswith("f16")
    n_deals = 2003 if three else 5001
    rng = np.random.Generator(np.random.PCG64(56))
    sizes = [(7, 9), (11, 8), (20011, 17003)] if three else [(30000, 16385)]
    n_actions, tree = rs.build_game_tree(rs.three_street_options() if three else rs.default_flop())
    table = rs.create_infosets(n_actions, tree, sizes, [1] * len(sizes), rs.F16 if half else rs.F32)
    otree = orc.OracleTree(orc.options_three_street() if three else orc.options_default_river())
    otab = orc.OracleDealTable(otree, sizes, orc.T_F16 if half else orc.T_F32)
    for nd in tree.action_nodes():
        a, n = nd.n_children, sizes[nd.round_idx][nd.player]
        R = rng.uniform(-1000, 1000, size=(a, n)).astype(np.float32)
        S = rng.uniform(0, 1000, size=(a, n)).astype(np.float32)
        R[:, ::5] = -0.0   # negative zeros where no deal may reach: the write-back makes them +0
        if half:
            R, S = R.astype(np.float16).astype(np.float32), S.astype(np.float16).astype(np.float32)
        table.upload_node(nd.index, R, S)
        otab.set_node(nd.index, R, S)
    cidx = {(r, p): rng.integers(0, sizes[r][p], size=n_deals).astype(np.uint32) for r in range(len(sizes)) for p in (0, 1)}
    sign = rng.integers(-1, 2, size=n_deals).astype(np.float32)
    sbuf = rs.deal_buffer(table, n_deals, sign)
    lg = {i: (rs.LEAF_SIGN, sbuf) for i, nd in enumerate(tree.nodes) if nd.kind == rs.NODE_TERMINAL and nd.ttype != rs.TERM_UNCONTESTED}
    lo = {i: (orc.LEAF_SIGN, sign) for i in lg}
    tr = rs.MCCFRTrainer(tree, table, lg, scale=0.25, mode=rs.UPD_CLAMP_I64 | rs.UPD_RMPLUS, fuse_subtrees=1, deals=cidx, opp_mode=rs.OPP_SAMPLE, sample_seed=5)
    osol = orc.OracleDealSolver(otree, otab, lo, cidx, n_deals, scale=0.25, mode=orc.UPD_CLAMP_I64, rmplus=True, opp_mode=orc.OPP_SAMPLE, base_seed=5)
    for it in range(3):
        for player in (0, 1):
            assert_bits(tr.iterate(player, want_root_util=True), osol.iterate(player), "root util it=%d p=%d" % (it, player))
    for nd in tree.action_nodes():
        r, s = table.download_node(nd.index)
        ro, so = otab.get_node(nd.index)
        assert_bits(r, ro, "regrets node %d" % nd.index)
        assert_bits(s, so, "ssum node %d" % nd.index)
    with pytest.raises(rs.RsError):   # pruning compares i32 regrets with the threshold (cfr.rs:352): not on float tables
        rs.MCCFRTrainer(tree, table, lg, scale=0.25, mode=rs.UPD_CLAMP_I64 | rs.UPD_PRUNE, fuse_subtrees=1, deals=cidx, opp_mode=rs.OPP_SAMPLE, sample_seed=5)
