"""GPU (-m gpu): the readers of the average strategy pinned where tests/test_gpu_br.py leaves them free.

  * the trainer's exploitability (rs_deal_trainer_best_response): board, run-outs, cluster ids per (round, prefix, hand) and their cache -- against the C oracle fed with
    the downloaded table and cluster ids computed HERE (canonical hand index of hole cards + board prefix, mapped through the abstraction's key order; never
    rs_card_abs_get_cluster), bit for bit in all four modes, and against oracle/np_br.py within f64 rounding.  The two players' ranges differ in size and overlap in part.
  * the shapes rs_br.hip branches on: every form of the rank-order leaf loop (ranges up to 256 / 512 / 1 024 / beyond, and a 10-against-1 081 pair), the own-node forms
    (info sets of 1, 8, 9, 64, 65 lanes side by side; lanes at 32 x clusters - 1, at it and one above; empty clusters; one cluster holding every lane; one-hand ranges).
  * numeric edges of the strategy sums through final_sigma: i32 at 2^31-1, around 2^24 and negative; f32 sums that overflow, +inf, NaN, -0.0, subnormals; binary16 at
    65 504, +inf, subnormals.  NaN results are compared by NaN-ness, everything else by bits.
Which kernel forms a case launches depends on its sizes AND its cluster layout (rs_br.hip br_prepare / BrRun::own_kind); the trainer cases assert br_launches(), and NOTES.md records the
kernels that one traced run of every case of the second group launched."""
import os

import numpy as np
import pytest

import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from oracle import orc
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from test_np_br_cpu import ATOL, MARGIN, RIVER, RTOL, TURN, check_margins, exact_tie_game, combos_of, disjoint_ranges, pick_ranges, prefixes_of, random_cids, sizes_of

pytestmark = pytest.mark.gpu

MODES = (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED)
GDT = {"i32": L.I32, "f32": L.F32, "f16": L.F16}
ODT = {"i32": orc.T_I32, "f32": orc.T_F32, "f16": orc.T_F16}
NPDT = {"i32": np.int32, "f32": np.float32, "f16": np.float16}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


class depth_first:
    """RS_BR_DEPTH_FIRST=1 for the calls inside: one launch per node instead of the level plan"""

    def __enter__(self):
        os.environ["RS_BR_DEPTH_FIRST"] = "1"

    def __exit__(self, *exc):
        del os.environ["RS_BR_DEPTH_FIRST"]


def same(got, want, what):
    """finite values by bits, NaN by NaN-ness (not payload)"""
    got, want = np.asarray(got), np.asarray(want)
    assert (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    ok = ~np.isnan(want)
    assert got[ok].tobytes() == want[ok].tobytes(), (what, got, want)


def close(got, want, what):
    assert (np.isnan(got) == np.isnan(want)).all(), (what, got, want)
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=RTOL, atol=ATOL), (what, got, want)


# ---- B. the trainer's exploitability ----------------------------------------------------------------------------------------------------------------

def python_cluster_ids(mask, ranges, card_abs, files):
    """cids[r][p][prefix, hand] of the trainer's game without get_cluster: the board is the mask's cards ascending (cfr.rs:108-112), round r sees them and the first r new
    cards of the run-out; the info set is the canonical index of (hole cards | those board cards) (card_abstraction.rs:204-209), through the bucket file where there is one
    (:287-292), mapped to its dense id by the abstraction's key order.  Lanes whose hand holds a new card are no deal: id 0."""
    board0 = [c for c in range(52) if mask >> c & 1]
    ro = nbr.runouts(board0)
    first = len(board0) - 3
    out = []
    for r, pf in enumerate(prefixes_of(board0)):
        street = first + r
        ix = orc.HandIndexer([2, 3 + street])
        per = len(ro) // pf
        row = []
        for p in (0, 1):
            keys = ix.generate_map(ranges[p], mask, 3 + street, files[r])
            assert (keys == card_abs[r].keys(p)).all() and len(keys) == card_abs[r].get_size(p)
            dense = {int(k): i for i, k in enumerate(keys)}
            ids = np.zeros((pf, len(ranges[p])), dtype=np.uint32)
            for f in range(pf):
                prefix = [int(c) for c in ro[f * per][: len(board0) + r]]
                for h, (c0, c1) in enumerate(ranges[p]):
                    if int(c0) in prefix[len(board0):] or int(c1) in prefix[len(board0):]:
                        continue
                    key = ix.get_index(np.array([c0, c1] + prefix, dtype=np.uint8))
                    ids[f, h] = dense[int(files[r][key]) if files[r] is not None else key]
            row.append(ids)
        out.append(row)
    return board0, out


def load_oracle(tr, otab, tree):
    sums = {}
    for nd in tree.action_nodes():
        R, S = tr.infosets.download_node(nd.index)
        otab.set_node(nd.index, R, S)
        sums[nd.index] = S
    return sums


def trainer_against_oracle(tr, tree, ot, sizes, dtype, board0, ranges, cids, nodes, modes=MODES, with_np_br=True, launches=None):
    otab = orc.OracleDealTable(ot, sizes, dtype=ODT[dtype])
    sums = load_oracle(tr, otab, tree)
    got = {}
    for mode in modes:
        got[mode] = tr.best_response(mode)
        if launches is not None:                                     # the level plan's launches of this call: both traversers
            n = tr.br_launches(bool(mode & L.BR_SORTED))
            assert n == launches[mode], (mode, n, launches[mode])
        same(got[mode], otab.best_response_rounds(board0, ranges[0], ranges[1], cids, mode), ("trainer against the oracle", mode))
    if with_np_br:
        sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
        game = nbr.Game(board0, ranges)
        for mode, name in ((L.BR_MAX, "max"), (L.BR_AVERAGE, "avg")):
            want = nbr.best_response(nodes, sig.__getitem__, board0, ranges, cids, name, None, game)
            close(got[mode], want, ("trainer against np_br", mode))
    assert tr.exploitability() == got[L.BR_MAX | L.BR_SORTED].sum() / 2.0
    return got


TRAINER_CASES = {
    # name: (board, hands of player 0 and 1, bucketed rounds, cell type, depth first)
    "river_lossless_i32": ("4d5dAs3cKs", 60, 45, (), "i32", False),
    "turn_bucketed_f32": ("4d5dAs3c", 40, 31, (0,), "f32", False),
    "turn_lossless_i32_depth_first": ("4d5dAs3c", 33, 40, (), "i32", True),
    "flop_bucketed_f16": ("7h8hQc", 12, 15, (0, 1), "f16", False),
    "flop_lossless_i32": ("7h8hQc", 14, 11, (), "i32", False),
}

# br_launches() after each mode's call in the level-plan cases: the launches of both traversers.  Which nodes share a launch is host logic alone (tree depth, kind, round, the
# 16 384-leaf slices), so the counts are exact.  Recorded on the GPU at commit afa54d2, before the level plan and the depth-first walk shared one job table and one launcher.
TRAINER_LAUNCHES = {
    "flop_bucketed_f16": dict(zip(MODES, (43, 48, 43, 48))),
    "flop_lossless_i32": dict(zip(MODES, (44, 49, 44, 49))),
    "river_lossless_i32": dict(zip(MODES, (9, 11, 9, 11))),
    "turn_bucketed_f32": dict(zip(MODES, (24, 28, 24, 28))),
}


@pytest.mark.parametrize("name", sorted(TRAINER_CASES))
def test_trainer_best_response_equals_oracle_and_np_br(name):
    """after a few batches, after more training (the cached ids against a changed table) and after br_release()"""
    text, n0, n1, bucketed, dtype, dfs = TRAINER_CASES[name]
    rng = np.random.Generator(np.random.PCG64(len(name) + n0))
    mask = ab.card_mask(text)
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.choice(len(allh), n, replace=False))] for n in (n0, n1)]
    ranges[1][: n1 // 3] = ranges[0][: n1 // 3]                      # a partial overlap, whatever the draw gave
    ranges[1] = np.unique(ranges[1], axis=0)
    shared = len(set(map(tuple, ranges[0])) & set(map(tuple, ranges[1])))
    assert 0 < shared < min(len(ranges[0]), len(ranges[1])) and len(ranges[0]) != len(ranges[1])
    n_board = bin(mask).count("1")
    rounds = 6 - n_board
    file_size = {0: 1286792, 1: 13960050}
    files = [(np.arange(file_size[n_board - 3 + r], dtype=np.uint64) * 2654435761 % (23 + 14 * r)).astype(np.uint32) if r in bucketed else None for r in range(rounds)]
    bets, raises = ((0.5,),) * rounds, ((),) * rounds
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises))
    card_abs = [ab.CardAbstraction.init(ranges, mask, n_board - 3 + r, files[r]) for r in range(rounds)]
    kw = {} if dtype == "i32" else dict(prune_threshold=None, scale=0.5)
    tr = rs.DealTrainer(tree, card_abs, ranges, mask, 1 << 12, seed=9, discount_interval=0, dtype=GDT[dtype], **kw)
    board0, cids = python_cluster_ids(mask, ranges, card_abs, files)
    sizes = [(card_abs[r].get_size(0), card_abs[r].get_size(1)) for r in range(rounds)]
    ot = orc.OracleTree(orc.make_options(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises))
    nodes, _ = npr.build_tree(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises)
    assert len(nodes) == ot.n_nodes

    def round_trip():
        if dfs:
            with depth_first():
                got = trainer_against_oracle(tr, tree, ot, sizes, dtype, board0, ranges, cids, nodes)
                assert tr.br_launches() == -1
        else:
            got = trainer_against_oracle(tr, tree, ot, sizes, dtype, board0, ranges, cids, nodes, launches=TRAINER_LAUNCHES[name])
            assert tr.br_launches() > 0                              # the level plan ran
        return got

    tr.train(3)
    tr.status()
    first = round_trip()
    tr.train(5)
    tr.status()
    second = round_trip()
    assert second[L.BR_MAX].tobytes() != first[L.BR_MAX].tobytes()   # the table did change under the cached ids
    tr.br_release()
    third = round_trip()
    assert all(third[m].tobytes() == second[m].tobytes() for m in MODES)
    tr.destroy()


def test_full_range_turn_game_sorted_against_the_oracle():
    """the form-3 leaf loop (1 128 combos a side, 48 run-outs, leaf slicing) of test_gpu_br.test_sorted_showdowns_full_ranges_from_a_flop, here against the oracle's
    rank-order mode bit for bit (the pair loop is what that test compares it with)"""
    mask = ab.card_mask("7h8hQc2d")
    hands = ab.random_range(mask)
    assert len(hands) == 1128
    bets, raises = ((1.0,), (1.0,)), ((), ())
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=4, bet_sizes=bets, raise_sizes=raises))
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, r, None) for r in (ab.TURN, ab.RIVER)]
    tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, 1 << 14, seed=6, discount_interval=0)
    tr.train(3)
    tr.status()
    board0, cids = python_cluster_ids(mask, [hands, hands], card_abs, [None, None])
    sizes = [(card_abs[r].get_size(0), card_abs[r].get_size(1)) for r in range(2)]
    ot = orc.OracleTree(orc.make_options(n_board_cards=4, bet_sizes=bets, raise_sizes=raises))
    trainer_against_oracle(tr, tree, ot, sizes, "i32", board0, [hands, hands], cids, None, modes=(L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED), with_np_br=False)
    assert tr.br_launches() > 0
    tr.destroy()


# ---- C and D: tables filled by hand ------------------------------------------------------------------------------------------------------------------

def plain_sums(rng, shape, dtype):
    S = rng.integers(0, 1000, shape).astype(np.float64)
    S[rng.random(shape) < 0.15] = 0
    return S.astype(NPDT[dtype])


def table_case(board0, h, cids, bets, raises, dtype, make_sums, seed, sizes=None, modes=MODES, with_np_br=True, margins=True, both_plans=True):
    """device against oracle (bits / NaN-ness) in `modes`, level plan and depth first; the pair-loop modes against np_br"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = sizes or sizes_of(cids)
    n_actions, tree = rs.build_game_tree(rs.Options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    table = rs.create_infosets(n_actions, tree, sizes, [1] * len(cids), dtype=GDT[dtype])
    ot = orc.OracleTree(orc.make_options(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises))
    otab = orc.OracleDealTable(ot, sizes, dtype=ODT[dtype])
    sums = {}
    for nd in tree.action_nodes():
        S = make_sums(rng, otab.node_shape(nd.index), dtype, nd)
        table.upload_node(nd.index, np.zeros(S.shape, dtype=NPDT[dtype]), S)
        otab.set_node(nd.index, np.zeros(S.shape), S)
        sums[nd.index] = S
    want = {mode: otab.best_response_rounds(board0, h[0], h[1], cids, mode) for mode in modes}
    got = {}
    for mode in modes:
        got[mode] = table.best_response_rounds(tree, board0, h[0], h[1], cids, mode)
        same(got[mode], want[mode], ("level plan", mode))
    if both_plans:
        with depth_first():
            for mode in modes:
                same(table.best_response_rounds(tree, board0, h[0], h[1], cids, mode), want[mode], ("depth first", mode))
    if len(board0) == 5 and sizes == sizes_of(cids):     # the single-round entry point takes the same game
        for mode in modes:
            if not mode & L.BR_SORTED:
                same(table.best_response(tree, board0, h[0], cids[0][0][0], h[1], cids[0][1][0], mode), otab.best_response(board0, h[0], cids[0][0][0], h[1], cids[0][1][0], mode),
                     ("rs_best_response", mode))
    if with_np_br:
        nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises)
        sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
        game = nbr.Game(board0, h)
        m = [] if margins else None
        for mode, name in ((L.BR_MAX, "max"), (L.BR_AVERAGE, "avg")):
            if mode in modes:
                close(got[mode], nbr.best_response(nodes, sig.__getitem__, board0, h, cids, name, m if mode == L.BR_MAX else None, game), ("np_br", mode))
        if m is not None and L.BR_MAX in modes:
            if margins == "edges":      # a pool of a dozen cell values: exact ties are expected where reach vanishes; none may be visible, the rest clear of rounding
                assert not any(x["visible_tie"] for x in m)
                assert min(x["margin"] / x["scale"] for x in m if x["margin"] > 0 and x["scale"] > 0) > MARGIN
            else:
                check_margins(m)
    return got


def blocks_cids(n, n_clusters):
    """hands in consecutive blocks of equal size: coarse info sets with many lanes each"""
    return (np.arange(n, dtype=np.uint32) * n_clusters // n).astype(np.uint32)[None, :]


LEAF_CASES = {
    # (hands of player 0, of player 1): the leaf-loop form is picked by the larger range (<= 256: 0, <= 512: 1, <= 1 024: 2, else 3), its LDS sized by the opponent's.
    # Player 0 has n0 // 32 info sets (32 x clusters at, one above and, 255, one below the lanes: thread per info set against wave, groups against columns); player 1 has
    # one info set holding every lane in a table of three (two empty clusters)
    "255": (255, 255), "256": (256, 256), "257": (257, 257), "512": (512, 512), "513": (513, 513), "1024": (1024, 1024), "1025": (1025, 1025), "1081": (1081, 1081),
    "10_1081": (10, 1081), "1081_10": (1081, 10),
}


@pytest.mark.parametrize("name", sorted(LEAF_CASES))
def test_leaf_loop_forms_on_a_full_board(name):
    n0, n1 = LEAF_CASES[name]
    rng = np.random.Generator(np.random.PCG64(n0 * 3 + n1))
    h = pick_ranges(rng, RIVER, n0, n1)
    nc0 = max(1, (n0 + 31) // 32 if n0 == 255 else n0 // 32)
    cids = [[blocks_cids(n0, nc0), np.full((1, n1), 2, dtype=np.uint32)]]
    table_case(RIVER, h, cids, ((0.5, 1.0),), ((3.0,),), "i32", lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype), n0 + n1, sizes=[(nc0, 3)])


@pytest.mark.parametrize("n0,n1", [(300, 420), (600, 700)])
def test_leaf_loop_forms_1_and_2_over_48_runouts(n0, n1):
    """turn start: the level plan slices the leaves over 48 run-outs; ranges in 257..512 take form 1, in 513..1 024 form 2.  Rank-order modes against the oracle's (its pair
    loop costs seconds at this size and is left out), level plan and depth first"""
    rng = np.random.Generator(np.random.PCG64(n0 + n1))
    h = pick_ranges(rng, TURN, n0, n1)
    cids = random_cids(rng, TURN, h, [(9, 7), (40, 50)])
    got = table_case(TURN, h, cids, ((0.5,), (1.0,)), ((), ()), "i32", lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype), n0,
                     modes=(L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED), with_np_br=False)
    assert abs(got[L.BR_AVERAGE | L.BR_SORTED].sum()) < 1e-9


def lane_partition_cids(game, p, sizes_cycle, rng=None):
    """last-round info sets cut from the dealt lanes in runs of sizes_cycle lanes: exact info-set sizes in a multi-round game.  The lanes are taken run-out major, hand
    minor, or, with `rng`, in a random order, so that every info set draws its lanes from distant run-outs"""
    dealt = ~game.blocked[p]
    lanes = np.argwhere(dealt)
    if rng is not None:
        lanes = lanes[rng.permutation(len(lanes))]
    ends = np.cumsum([sizes_cycle[i % len(sizes_cycle)] for i in range(len(lanes) // min(sizes_cycle) + 1)])
    ids = np.zeros(dealt.shape, dtype=np.uint32)
    ids[lanes[:, 0], lanes[:, 1]] = np.searchsorted(ends, np.arange(len(lanes)), side="right")
    return ids


def runout_components(ids, dealt):
    """sizes of the classes of run-outs that info sets tie together (two run-outs holding lanes of one info set belong together): what build_groups of rs_br.hip packs"""
    parent = list(range(ids.shape[0]))

    def find(b):
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        return b

    first = {}
    for b, hh in np.argwhere(dealt):
        a = find(first.setdefault(int(ids[b, hh]), int(b)))
        parent[find(int(b))] = a
    return sorted(np.bincount([find(b) for b in range(len(parent))]).tolist(), reverse=True)


def test_own_node_info_sets_of_1_8_9_64_65_lanes():
    """the 8-lane fast path of k_br_own and its neighbours side by side in one node, on a full board (147 hands = 1 + 8 + 9 + 64 + 65, two empty clusters after them) and
    in the river round of a turn-start game (every dealt lane in runs of 1, 8, 9, 64, 65)"""
    cut = np.repeat(np.arange(5, dtype=np.uint32), [1, 8, 9, 64, 65])[None, :]
    rng = np.random.Generator(np.random.PCG64(147))
    h = pick_ranges(rng, RIVER, 147, 200)
    fill = lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype)
    table_case(RIVER, h, [[cut, blocks_cids(200, 5)]], ((0.5, 1.0),), ((3.0,),), "i32", fill, 1, sizes=[(7, 5)])
    table_case(RIVER, [h[1], h[0]], [[blocks_cids(200, 5), cut]], ((0.5, 1.0),), ((3.0,),), "i32", fill, 2, sizes=[(5, 7)])
    h = pick_ranges(rng, TURN, 30, 26)
    game = nbr.Game(TURN, h)
    cids = random_cids(rng, TURN, h, [(4, 3), (1, 1)])
    cids[1] = [lane_partition_cids(game, p, [1, 8, 9, 64, 65]) for p in (0, 1)]
    table_case(TURN, h, cids, ((0.5,), (1.0,)), ((), ()), "i32", fill, 3)


def test_thread_per_info_set_in_max_mode_under_the_level_plan_with_8_and_9_lanes():
    """k_br_own_jobs and its 8-lane fast path in BR_MAX mode under the LEVEL plan -- the route every bucketed abstraction takes in exploitability().  300 hands a side
    from the turn; the river info sets are runs of 8 and 9 lanes cut from a random order of all dealt lanes, so every one spans distant run-outs and all 48 run-outs form ONE
    component (asserted): more than the 11 264 // 300 = 37 run-outs a group may hold, so build_groups gives up for both players; the lanes (14 400) are fewer than 32 x info
    sets (asserted), so neither the columns nor the wave form is asked and rs_br.hip's own_kind takes the thread per info set in both modes.  (Where a round IS taken by
    groups, only BR_MAX goes by groups; BR_AVERAGE falls through to the same thread-per-info-set kernel.)"""
    rng = np.random.Generator(np.random.PCG64(89))
    h = pick_ranges(rng, TURN, 300, 300)
    game = nbr.Game(TURN, h)
    cids = random_cids(rng, TURN, h, [(6, 5), (1, 1)])
    cids[1] = [lane_partition_cids(game, p, [8, 9], rng) for p in (0, 1)]
    for p in (0, 1):
        sizes = np.bincount(cids[1][p][~game.blocked[p]])
        assert set(sizes[:-1].tolist()) == {8, 9} and 1 <= sizes[-1] <= 9
        assert runout_components(cids[1][p], ~game.blocked[p])[0] > 11264 // 300       # kBrGroupPerThread * kBrGroupBlock / n_hands: build_groups gives up
        assert 48 * 300 < 32 * (int(cids[1][p].max()) + 1)
    table_case(TURN, h, cids, ((0.5,), (1.0,)), ((), ()), "i32", lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype), 4)


def test_first_maximum_not_last_on_an_exact_tie_on_the_device():
    """test_np_br_cpu.exact_tie_game: river info sets of two lanes whose two actions tie exactly with different lanes, under turn info sets that tell the lanes apart.  The
    device takes the first maximum (cfr.rs:684-690) in every form -- bits of the oracle, level plan and depth first, pair loop and rank order -- and is far from what
    the last maximum gives (np_br with the wrong rule)"""
    board0, h, cids, bets, raises, nodes, sums = exact_tie_game()
    got = table_case(board0, h, cids, bets, raises, "i32", lambda rng, shape, dtype, nd: sums[nd.index], 0, margins=False)
    sig = {i: nbr.final_strategy(S) for i, S in sums.items()}
    last = nbr.best_response(nodes, sig.__getitem__, board0, h, cids, "max", None, None, "last")
    for mode in (L.BR_MAX, L.BR_MAX | L.BR_SORTED):
        assert last[0] > got[mode][0] + 10.0, (mode, got[mode], last)


# ranges of 1, 7, 8 and 9 hands: the reach kernels deal the hands out to eight slices (br_xcd_sliced_lane) -- slices that are empty, of one hand, and of one and two hands
SLICE_RANGES = [(1, 9), (7, 8), (8, 7), (9, 1)]


@pytest.mark.parametrize("n0,n1", [(1, 40), (40, 1), (1, 1)] + SLICE_RANGES)
def test_one_hand_ranges_from_the_turn(n0, n1):
    """a range of one hand on either side: two of the 48 turn cards block it (no deal in those run-outs: the lane carries nothing and belongs to no info set); and the
    ranges of SLICE_RANGES, hands that share no card, in both tree orders"""
    rng = np.random.Generator(np.random.PCG64(50 + n0))
    h = disjoint_ranges(rng, TURN, n0, n1) if (n0, n1) in SLICE_RANGES else pick_ranges(rng, TURN, n0, n1)
    if n0 == n1 == 1:
        h[1] = combos_of(TURN)[7:8] if tuple(h[0][0]) != tuple(combos_of(TURN)[7]) else combos_of(TURN)[900:901]
    cids = random_cids(rng, TURN, h, [(min(n0, 4), min(n1, 4)), (3, 5)])
    table_case(TURN, h, cids, ((0.5,), (1.0,)), ((), ()), "i32", lambda rng, shape, dtype, nd: plain_sums(rng, shape, dtype), 60 + n1, sizes=[(min(n0, 4), min(n1, 4)), (3, 5)],
               margins="edges")


# ---- D. numeric edges ----------------------------------------------------------------------------------------------------------------------------------

def edge_sums(rng, shape, dtype, poison=False):
    """finite edges in every node; with `poison`, +inf cells (inf / inf = NaN) in the columns of cluster 1"""
    A, n = shape
    if dtype == "i32":
        pool = np.array([2**31 - 1, 2**31 - 1, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 1, 0, 0, -1, -(2**31), 977, 31], dtype=np.int64)
        S = pool[rng.integers(0, len(pool), shape)]
        S[:, rng.random(n) < 0.1] = -rng.integers(1, 1000, (A, 1))      # all-negative columns: uniform
        return S.astype(np.int32)
    if dtype == "f32":
        pool = np.array([3.4e38, 3.0e38, 1.7e38, 1.0, 977.25, 0.0, -0.0, 1e-45, 3e-45, 1.1754942e-38, -5.0, np.nan, 2.0**24 + 2], dtype=np.float32)
    else:
        pool = np.array([65504.0, 65504.0, 32768.0, 1.0, 977.0, 0.0, -0.0, 6e-8, 1.8e-7, 6.1e-5, -5.0, np.nan, 2049.0], dtype=np.float16)
    S = pool[rng.integers(0, len(pool), shape)]
    if poison and n > 1:
        S[0, 1] = np.inf
    return S.astype(NPDT[dtype])


@pytest.mark.parametrize("dtype", ["i32", "f32", "f16"])
@pytest.mark.parametrize("board0", [RIVER, TURN], ids=["river", "turn"])
def test_finite_edges_of_the_strategy_sums(dtype, board0):
    """every result stays finite: an f32 column whose positive sum overflows plays nothing (finite / inf = 0), NaN cells are not positive (not played, not summed), -0.0 and
    negative cells likewise, subnormals divide as IEEE says, binary16 cells at 65 504 add up in f32.  i32 cells at 2^31-1 and around 2^24 round `as f32`"""
    rng = np.random.Generator(np.random.PCG64(len(board0)))
    rounds = 6 - len(board0)
    h = pick_ranges(rng, board0, 61, 47)
    cids = random_cids(rng, board0, h, [(6, 5), (9, 7)][:rounds])
    got = table_case(board0, h, cids, ((0.5, 1.0),) * rounds, ((3.0,),) * rounds, dtype, lambda rng, shape, dtype, nd: edge_sums(rng, shape, dtype), 5, margins="edges")
    assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("board0", [RIVER, TURN], ids=["river", "turn"])
def test_poisoned_columns_reach_what_they_should(dtype, board0):
    """+inf in action 0 of cluster 1 of every node of PLAYER 1's first round: its final strategy there is NaN (inf / inf) for action 0 and 0 for the others.
    Expected reach -- BR_MAX: player 1 as the traverser never reads its own strategy, so out[1] stays finite; as the opponent its reach is NaN on every lane of cluster 1
    from its first node on, which is the child of player 0's first action at the root (asserted below): the sum of that action is NaN in every info set of player 0 that meets such a lane, NaN
    is never the smaller side of cfr.rs:686's strict <, so the first action stays chosen and out[0] is NaN.  BR_AVERAGE: both are NaN (player 1 plays the NaN itself).
    The same cells in a cluster no lane belongs to reach nothing."""
    rng = np.random.Generator(np.random.PCG64(len(board0) + 7))
    rounds = 6 - len(board0)
    h = pick_ranges(rng, board0, 40, 37)
    bets, raises = ((0.5,),) * rounds, ((),) * rounds

    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=bets, raise_sizes=raises)
    root = nodes[nodes[0]["children"][0]]
    assert root["player"] == 0 and nodes[root["children"][0]]["kind"] == "action" and nodes[root["children"][0]]["player"] == 1 and nodes[root["children"][0]]["round_idx"] == 0

    def fill(rng, shape, dtype, nd):
        return edge_sums(rng, shape, dtype, poison=(nd.player == 1 and nd.round_idx == 0))

    cids = random_cids(rng, board0, h, [(6, 5), (9, 7)][:rounds])
    got = table_case(board0, h, cids, bets, raises, dtype, fill, 9, margins=False)      # the margins are NaN wherever the poison reaches
    for mode in MODES:
        if mode & 0xff == L.BR_MAX:
            assert np.isnan(got[mode][0]) and np.isfinite(got[mode][1]), (mode, got[mode])
        else:
            assert np.isnan(got[mode]).all(), (mode, got[mode])
    cids[0][1][cids[0][1] == 1] = 0                       # nobody is in cluster 1 any more
    got = table_case(board0, h, cids, bets, raises, dtype, fill, 9, sizes=[(6, 5), (9, 7)][:rounds], margins=False)
    assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("dtype", ["i32", "f32", "f16"])
@pytest.mark.parametrize("river", [True, False])
def test_calc_br_at_the_edges(dtype, river):
    """rs_calc_br reads bucket 0 of every node through the same final_sigma: device, C oracle and the Python restatement (on np_br's final strategy) on edge cells"""
    n_actions, tree = rs.build_game_tree(rs.default_flop() if river else rs.three_street_options())
    rounds = 1 if river else 3
    ot = orc.OracleTree(orc.options_default_river() if river else orc.options_three_street())
    nodes, _ = npr.build_tree() if river else npr.build_tree(n_board_cards=3, bet_sizes=((0.5, 1.0),) * 3, raise_sizes=((3.0,),) * 3)
    for seed in range(6):
        rng = np.random.Generator(np.random.PCG64(seed))
        table = rs.create_infosets(n_actions, tree, [3] * rounds, [1] * rounds, dtype=GDT[dtype])
        otab = orc.OracleTable(ot, [1] * rounds, 3, ODT[dtype])
        sig0 = {}
        for nd in tree.action_nodes():
            S = edge_sums(rng, otab.node_shape(nd.index), dtype, poison=seed >= 4)
            if seed >= 4 and dtype != "i32":
                S[0, 0] = np.inf if nd.index % 5 == 0 else S[0, 0]
            table.upload_node(nd.index, np.zeros(S.shape, dtype=NPDT[dtype]), S)
            otab.set_node(nd.index, np.zeros(S.shape), S)
            sig0[nd.index] = nbr.final_strategy(S)[:, 0]
        got, want = table.calc_br(tree), otab.calc_br()
        same(got, want, (dtype, river, seed))
        same(want, npr.calc_br(nodes, sig0), ("restated", dtype, river, seed))
