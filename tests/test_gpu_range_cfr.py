"""GPU (-m gpu): full-width CFR over hand ranges (rs_range_cfr_*, rs_deal_trainer_range_cfr) and RS_BR_CURRENT against the numpy restatement tests/np_range_cfr.py.

Every comparison with the restatement is TEACHER-FORCED: its tables are uploaded, the device does one sweep, and the result is compared with the restatement's own next
state -- rounding cannot build up.  A cell passes if it is of the restatement's class (finite, +inf, -inf, NaN) and, where finite, within one f32 ulp of the restatement's
or within ATOL absolutely (test_range_cfr_cpu.compare_cells; on well-behaved tables that file holds two orders of the same sums to one ulp with no ATOL, on edge
tables to this rule); at most 0.5 % of a case's cells may differ at all; cells a sweep must not touch are bit-equal to what was uploaded.
The shapes are the smallest at which each branch of rs_br.hip's new kernels can go wrong (BrRun::own_kind: a wave per info set from 32 lanes per cluster on);
tests/test_gpu_range_cfr_edges.py goes on to list lengths at the kernels' steps, wide nodes, three rounds and tables of edge values."""
import numpy as np
import pytest

import np_range_cfr as nrc
import rustsolver_amd as rs
from oracle import np_br as nbr
from oracle import np_restate as npr
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from test_gpu_br_pinned import GDT, MODES, SLICE_RANGES, TRAINER_CASES, close, depth_first, edge_sums, python_cluster_ids
from test_np_br_cpu import ATOL, RIVER, RTOL, TURN, combos_of, disjoint_ranges, lane_cids, pick_ranges, random_cids, sizes_of
from test_range_cfr_cpu import RIVER_TREE, TURN_TREE, adopt_tree, compare_cells, random_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def runs_cids(board0, h, runs):
    """last (only) round info sets cut from the hands in runs of the given lengths, one prefix"""
    assert len(board0) == 5
    return [[np.repeat(np.arange(len(r), dtype=np.uint32), r)[None, :] for r in runs]]


def no_opponent_game():
    """player 1 holds only combos with the ace of hearts; player 0's combos with that card meet no opponent at all (weight 0 on every lane)"""
    rng = np.random.Generator(np.random.PCG64(5))
    ah = 4 * 12 + 1
    combos = combos_of(TURN)
    with_ah, rest = combos[(combos == ah).any(axis=1)], combos[~(combos == ah).any(axis=1)]
    return [np.concatenate([with_ah[:2], rest[np.sort(rng.choice(len(rest), 8, replace=False))]]), with_ah[5:9]]


def make_case(name):
    """-> board0, hands, cids, table sizes, (bet sizes, raise sizes)"""
    rng = np.random.Generator(np.random.PCG64(7))
    if name == "river_lanes":                       # thread form, info sets of one lane
        h = pick_ranges(rng, RIVER, 25, 20)
        cids = lane_cids(RIVER, h)
        return RIVER, h, cids, sizes_of(cids), RIVER_TREE
    if name == "river_wave_35":                     # wave form (70 >= 2 x 32, 66 >= 2 x 32): lists of ~35 lanes, shorter than one step
        h = pick_ranges(rng, RIVER, 70, 66)
        return RIVER, h, random_cids(rng, RIVER, h, [(2, 2)]), [(2, 2)], RIVER_TREE
    if name == "river_runs_8_9":                    # thread form: info sets of 8 and 9 lanes side by side, a single lane and a second 8
        h = pick_ranges(rng, RIVER, 26, 26)
        return RIVER, h, runs_cids(RIVER, h, ([8, 9, 1, 8], [9, 8, 9])), [(4, 3)], RIVER_TREE
    if name == "turn_imperfect_recall":             # wave form: lists beyond 64 and 128 lanes, blocked lanes, imperfect recall
        h = pick_ranges(rng, TURN, 9, 7)
        return TURN, h, random_cids(rng, TURN, h, [(3, 4), (5, 6)]), [(3, 4), (5, 6)], TURN_TREE
    if name == "turn_lanes":                        # thread form over 48 run-outs
        h = pick_ranges(rng, TURN, 9, 7)
        cids = lane_cids(TURN, h)
        return TURN, h, cids, sizes_of(cids), TURN_TREE
    if name == "river_unused_cluster":              # cluster ids that no lane uses: the last of each player, and whatever the draw left out
        h = pick_ranges(rng, RIVER, 25, 20)
        return RIVER, h, random_cids(rng, RIVER, h, [(6, 9)]), [(8, 11)], RIVER_TREE
    if name == "turn_one_hand":                     # a range of one hand: two turn cards block it
        h = pick_ranges(rng, TURN, 1, 7)
        return TURN, h, random_cids(rng, TURN, h, [(1, 3), (2, 4)]), [(1, 3), (2, 4)], TURN_TREE
    if name in SLICES:                              # 1, 7, 8 and 9 hands a side: empty and uneven slices of the reach kernels' lane mapping (br_xcd_sliced_lane)
        n0, n1 = (int(x) for x in name.split("_")[2:])
        h = disjoint_ranges(rng, TURN, n0, n1)
        sizes = [(min(n0, 3), min(n1, 4)), (5, 6)]
        return TURN, h, random_cids(rng, TURN, h, sizes), sizes, TURN_TREE
    if name == "turn_no_opponent":
        h = no_opponent_game()
        return TURN, h, random_cids(rng, TURN, h, [(4, 2), (5, 3)]), [(4, 2), (5, 3)], TURN_TREE
    raise KeyError(name)


SLICES = ["turn_slices_%d_%d" % r for r in SLICE_RANGES]
CASES = ["river_lanes", "river_wave_35", "river_runs_8_9", "turn_imperfect_recall", "turn_lanes", "river_unused_cluster", "turn_one_hand", "turn_no_opponent"]
# the form of the LAST round's own nodes per player (wave per info set?).  turn_lanes' first round (9 and 7 info sets over 48 run-outs) is in the wave form all the
# same; test_gpu_range_cfr_edges.FORMS keys the forms per (round, player)
WAVE = {"river_wave_35": (True, True), "turn_imperfect_recall": (True, True), "river_lanes": (False, False), "turn_lanes": (False, False), "river_runs_8_9": (False, False)}


class Device:
    """the device side of a case: tree, f32 table, and one RangeCFR per (rmplus, sorted)"""

    def __init__(self, board0, h, cids, sizes, tree, dtype=L.F32):
        self.board0, self.h, self.cids = board0, h, cids
        if max(len(x) for x in tree[0] + tree[1]) <= L.MAX_SIZES:
            self.n_actions, self.tree = rs.build_game_tree(rs.Options(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1]))
        else:                                        # rs_options holds no more sizes per round: the restated tree, adopted
            self.tree = adopt_tree(npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])[0])
            self.n_actions = self.tree.n_action_nodes
        self.table = rs.create_infosets(self.n_actions, self.tree, sizes, [1] * len(cids), dtype=dtype)
        self.solvers = {}

    def solver(self, rmplus=False, sorted_showdowns=True):
        key = (rmplus, sorted_showdowns)
        if key not in self.solvers:
            self.solvers[key] = rs.RangeCFR(self.table, self.tree, self.board0, self.h[0], self.h[1], self.cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns)
        return self.solvers[key]

    def upload(self, R, S):
        for i in R:
            self.table.upload_node(i, R[i], S[i])

    def download(self):
        R, S = {}, {}
        for nd in self.tree.action_nodes():
            R[nd.index], S[nd.index] = self.table.download_node(nd.index)
        return R, S

    def close(self):
        for s in self.solvers.values():
            s.destroy()
        self.solvers = {}


def copy_tables(R, S):
    return {i: x.copy() for i, x in R.items()}, {i: x.copy() for i, x in S.items()}


def same_tables(a, b):
    return all(a[0][i].tobytes() == b[0][i].tobytes() and a[1][i].tobytes() == b[1][i].tobytes() for i in a[0])


def compare_sweep(nodes, game, cids, p, before, got, want, what):
    """cells of `got` (device) against `want` (restatement) after one sweep of traverser p from `before`; returns (cells, cells that differ at all, largest ulp distance of two cells further apart than ATOL)"""
    cells = differ = worst = 0
    for nd in nodes:
        if nd["kind"] != "action":
            continue
        i = nd["index"]
        C = before[0][i].shape[1]
        used = np.zeros(C, dtype=bool)
        if nd["player"] == p:
            used[np.unique(game.infoset_of(cids, nd["round_idx"], p)[~game.blocked[p]])] = True
        for k in (0, 1):
            g, w, b = got[k][i], want[k][i], before[k][i]
            assert g[:, ~used].tobytes() == b[:, ~used].tobytes(), (what, "a cell the sweep must not touch changed", i, k)
            d, far = compare_cells(g[:, used], w[:, used], (what, i, k))
            cells += d.size
            differ += int((d > 0).sum())
            worst = max(worst, int(far.max()) if d.size else 0)
    return cells, differ, worst


@pytest.mark.parametrize("name", CASES + SLICES)
def test_one_sweep_equals_the_restatement(name):
    """from random and from zero tables, both traversers, plain and RM+, rank-order and pair-loop leaves; the same call twice gives the same bits"""
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    game = nbr.Game(board0, h)
    if name in WAVE:                                 # the form the case is there for (rs_br.hip br_wave_per_info_set, last round)
        for p in (0, 1):
            lanes, n_clusters = len(game.ro) * len(h[p]), sizes[-1][p]
            assert (lanes >= 32 * n_clusters) == WAVE[name][p], (name, p, lanes, n_clusters)
    if name == "turn_no_opponent":
        assert (game.W[:, :2, :] == 0).all()
    dev = Device(board0, h, cids, sizes, tree)
    cells = differ = 0
    for start in ("random", "zero"):
        for p in (0, 1):
            for rmplus in (False, True):
                rng = np.random.Generator(np.random.PCG64(100 + 2 * p + rmplus))
                before = random_tables(rng, nodes, sizes) if start == "random" else nrc.zero_tables(nodes, sizes)
                want = copy_tables(*before)
                value = nrc.sweep(nodes, want[0], want[1], game, cids, p, rmplus)
                for sorted_showdowns in (True, False):
                    what = (name, start, p, rmplus, sorted_showdowns)
                    dev.upload(*before)
                    got_value = dev.solver(rmplus, sorted_showdowns).iterate(p)
                    got = dev.download()
                    assert np.isclose(got_value, value, rtol=RTOL, atol=ATOL), (what, got_value, value)
                    c, d, _ = compare_sweep(nodes, game, cids, p, before, got, want, what)
                    cells, differ = cells + c, differ + d
                    if sorted_showdowns:             # determinism: the same call from the same tables
                        dev.upload(*before)
                        assert dev.solver(rmplus, True).iterate(p) == got_value
                        assert same_tables(dev.download(), got), what
    assert cells > 0 and differ <= 0.005 * cells, (name, differ, cells)
    assert dev.solver().nbytes > 0
    dev.close()


@pytest.mark.parametrize("name", ["turn_imperfect_recall", "turn_lanes"] + SLICES)
def test_level_plan_and_depth_first_walk_give_the_same_bits(name):
    board0, h, cids, sizes, tree = make_case(name)
    nodes, _ = npr.build_tree(n_board_cards=len(board0), bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    before = random_tables(np.random.Generator(np.random.PCG64(21)), nodes, sizes)
    for rmplus in (False, True):
        for sorted_showdowns in (True, False):
            dev.upload(*before)
            levels = dev.solver(rmplus, sorted_showdowns)
            v = [levels.iterate(0), levels.iterate(1)]
            assert levels.launches() > 0
            got = dev.download()
            with depth_first():
                walk = rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], cids, rmplus=rmplus, sorted_showdowns=sorted_showdowns)
                dev.upload(*before)
                w = [walk.iterate(0), walk.iterate(1)]
                assert walk.launches() == -1
            assert v == w, (name, rmplus, sorted_showdowns, v, w)
            assert same_tables(dev.download(), got), (name, rmplus, sorted_showdowns)
            walk.destroy()
    dev.close()


def test_train_with_dcfr_equals_sweeps_and_ticks_issued_one_by_one():
    """3 iterations with DCFR (1.5, 0, 2); and the same run split 2 + 1 with t0 = 2"""
    board0, h, cids, sizes, tree = make_case("river_unused_cluster")
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])
    dev = Device(board0, h, cids, sizes, tree)
    before = random_tables(np.random.Generator(np.random.PCG64(31)), nodes, sizes)
    for rmplus in (False, True):
        s = dev.solver(rmplus)
        dev.upload(*before)
        values = s.train(3, dcfr=True)
        whole = dev.download()
        dev.upload(*before)
        for t in (1, 2, 3):
            one = [s.iterate(0), s.iterate(1)]
            dev.table.discount_dcfr(*rs.dcfr_factors(1.5, 0.0, 2.0, t))
        assert same_tables(dev.download(), whole) and one == values.tolist()
        dev.upload(*before)
        s.train(2, dcfr=rs.dcfr_params(1.5, 0.0, 2.0))
        s.train(1, dcfr=rs.dcfr_params(1.5, 0.0, 2.0, t0=2))
        assert same_tables(dev.download(), whole)
        dev.upload(*before)
        s.train(3)
        assert not same_tables(dev.download(), whole)            # the ticks did something
    dev.close()


@pytest.mark.parametrize("algo,bound", [("cfr", 0.02), ("rmplus", 0.02), ("dcfr", 0.001)])
def test_200_iterations_solve_the_river_game(algo, bound):
    """river 25 x 20, one info set per hand, from zero tables: rs_best_response (RS_BR_MAX | RS_BR_SORTED) on the trained table against its value on the zero table.
    The restatement reaches 1.13 % (CFR), 1.02 % (RM+) and 0.037 % (DCFR); the margins allow for a trajectory that differs from it by rounding."""
    board0, h, cids, sizes, tree = make_case("river_lanes")
    dev = Device(board0, h, cids, sizes, tree)
    br = lambda: dev.table.best_response(dev.tree, board0, h[0], cids[0][0][0], h[1], cids[0][1][0], L.BR_MAX | L.BR_SORTED).sum()
    zero = br()
    assert abs(zero / 2.0 - 79.69) < 0.01
    values = dev.solver(algo == "rmplus").train(200, dcfr=True if algo == "dcfr" else None)
    trained = br()
    print(algo, "exploitability", zero / 2.0, "->", trained / 2.0, "share", trained / zero)
    assert trained < bound * zero, (algo, trained, zero)
    assert np.isfinite(values).all()
    dev.close()


def test_refused_calls_leave_the_table_alone():
    board0, h, cids, sizes, tree = make_case("river_unused_cluster")
    nodes, _ = npr.build_tree(n_board_cards=5, bet_sizes=tree[0], raise_sizes=tree[1])
    before = random_tables(np.random.Generator(np.random.PCG64(41)), nodes, sizes)
    for dtype in (L.I32, L.F16):
        dev = Device(board0, h, cids, sizes, tree, dtype=dtype)
        for i in before[0]:
            dev.table.upload_node(i, np.round(before[0][i]), np.round(before[1][i]))
        kept = dev.download()
        with pytest.raises(rs.RsError) as e:
            dev.solver()
        assert e.value.code == L.ERR_UNSUPPORTED
        assert same_tables(dev.download(), kept)
    dev = Device(board0, h, cids, sizes, tree)
    dev.upload(*before)
    kept = dev.download()
    _, other = rs.build_game_tree(rs.Options(n_board_cards=5, bet_sizes=((0.5,),), raise_sizes=((),)))
    with pytest.raises(rs.RsError) as e:                           # a tree whose action counts are not the table's
        rs.RangeCFR(dev.table, other, board0, h[0], h[1], cids)
    assert e.value.code in (L.ERR_INVALID, L.ERR_OOB)
    bad = [[cids[0][0].copy(), cids[0][1].copy()]]
    bad[0][1][0, 3] = sizes[0][1]                                  # one past the last cluster of player 1
    with pytest.raises(rs.RsError) as e:
        rs.RangeCFR(dev.table, dev.tree, board0, h[0], h[1], bad)
    assert e.value.code == L.ERR_OOB
    with pytest.raises(rs.RsError):
        dev.solver().iterate(2)
    assert same_tables(dev.download(), kept)
    dev.close()


def trainer_game(name):
    """the game of test_gpu_br_pinned's trainer case `name`: trainer, tree, restated nodes, board, ranges, cluster ids, table sizes"""
    text, n0, n1, bucketed, dtype, _ = TRAINER_CASES[name]
    rng = np.random.Generator(np.random.PCG64(len(name) + n0))
    mask = ab.card_mask(text)
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.choice(len(allh), n, replace=False))] for n in (n0, n1)]
    ranges[1][: n1 // 3] = ranges[0][: n1 // 3]
    ranges[1] = np.unique(ranges[1], axis=0)
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
    nodes, _ = npr.build_tree(n_board_cards=n_board, bet_sizes=bets, raise_sizes=raises)
    return tr, tree, nodes, board0, ranges, cids, sizes, dtype


def test_deal_trainer_trains_full_width_on_its_own_game():
    """DealTrainer(F32) on the turn_bucketed_f32 game: the trainer's cached cluster tables against ids computed here, sweep pair by sweep pair; exploitability falls; the
    sampled trainer goes on afterwards (kept shadow records were invalidated)"""
    tr, tree, nodes, board0, ranges, cids, sizes, dtype = trainer_game("turn_bucketed_f32")
    game = nbr.Game(board0, ranges)
    tr.train(3)
    tr.status()
    done = tr.iterations

    def tables():
        R, S = {}, {}
        for nd in tree.action_nodes():
            R[nd.index], S[nd.index] = tr.infosets.download_node(nd.index)
        return R, S

    cells = differ = 0
    for it in range(2):                                           # teacher-forced per iteration: both sweeps from the device's own tables
        before = tables()
        want = copy_tables(*before)
        values = tr.train_full_width(1, rmplus=bool(it))
        mid = copy_tables(*want)
        v0 = nrc.sweep(nodes, want[0], want[1], game, cids, 0, bool(it))
        after0 = copy_tables(*want)
        v1 = nrc.sweep(nodes, want[0], want[1], game, cids, 1, bool(it))
        assert np.allclose(values, [v0, v1], rtol=1e-6, atol=1e-9), (values, v0, v1)   # (traverser 1 reads regrets that may differ by an f32 ulp)
        got = tables()
        for p, (b, w) in enumerate(((mid, after0), (after0, want))):         # traverser p's nodes are written by sweep p alone
            own = [nd for nd in nodes if nd["kind"] == "action" and nd["player"] == p]
            c, d, _ = compare_sweep(own, game, cids, p, b, got, w, ("trainer", it, p))
            cells, differ = cells + c, differ + d
    assert cells > 0 and differ <= 0.005 * cells, (differ, cells)
    assert tr.iterations == done
    e0 = tr.exploitability()
    tr.train_full_width(20)
    e1 = tr.exploitability()
    print("exploitability", e0, "->", e1, "current", tr.exploitability(current=True))
    assert e1 < e0
    tr.train(1)
    tr.status()
    tr.destroy()


def br_current_case(name, draw):
    """regrets from draw(rng, shape, dtype) on the trainer's table: all four modes | RS_BR_CURRENT against np_br fed with get_strategy of the regrets as stored; the modes
    without the bit return the same bits before and after.  Returns the values with the bit"""
    tr, tree, nodes, board0, ranges, cids, sizes, dtype = trainer_game(name)
    tr.train(2)
    tr.status()
    rng = np.random.Generator(np.random.PCG64(77))
    sig = {}
    for nd in tree.action_nodes():
        R, S = tr.infosets.download_node(nd.index)
        tr.infosets.upload_node(nd.index, draw(rng, R.shape, dtype), S)
        Rn, _ = tr.infosets.download_node(nd.index)              # as stored (binary16 cells round)
        with np.errstate(over="ignore", invalid="ignore"):
            sig[nd.index] = npr.get_strategy(Rn) if dtype == "i32" else npr.get_strategy_f32(Rn)
    plain = {m: tr.best_response(m) for m in MODES}
    game = nbr.Game(board0, ranges)
    want = {"max": nbr.best_response(nodes, sig.__getitem__, board0, ranges, cids, "max", None, game),
            "avg": nbr.best_response(nodes, sig.__getitem__, board0, ranges, cids, "avg", None, game)}
    out = {}
    for m in MODES:
        got = out[m] = tr.best_response(m | L.BR_CURRENT)
        close(got, want["avg" if m & 0xff == L.BR_AVERAGE else "max"], (name, m))
        assert tr.best_response(m, current=True).tobytes() == got.tobytes()
        assert got.tobytes() != plain[m].tobytes()
    real = tr.best_response(L.BR_MAX | L.BR_REAL | L.BR_SORTED | L.BR_CURRENT)
    assert (real >= want["max"] - 1e-9).all()                     # the real game's responder is never worse off
    assert abs(want["avg"].sum()) < 1e-9
    for m in MODES:
        assert tr.best_response(m).tobytes() == plain[m].tobytes()
    tr.destroy()
    return out


def random_regrets(rng, shape, dtype):
    if dtype == "i32":
        return rng.integers(-1000, 1000, shape).astype(np.int32)
    return np.round(rng.standard_normal(shape) * 30.0, 1).astype(np.float32)


@pytest.mark.parametrize("name", sorted(TRAINER_CASES))
def test_br_current_reads_get_strategy_of_the_regrets(name):
    """random regrets on the trainer's table: all four modes | RS_BR_CURRENT against np_br fed with get_strategy of the regrets; the modes without the bit return the same
    bits before and after"""
    br_current_case(name, random_regrets)


@pytest.mark.parametrize("name", sorted(TRAINER_CASES))
def test_br_current_reads_get_strategy_of_edge_regrets(name):
    """the regret reader where test_gpu_br_pinned.edge_sums pins the strategy-sum reader: i32 cells around 2^24, at INT_MAX and INT_MIN (`as f32`), f32 columns whose
    positive sum overflows (they play nothing), binary16 cells of 65 504 added in f32, subnormals, -0.0 and NaN (not positive).  No +inf cell: every value is finite"""
    out = br_current_case(name, edge_sums)
    assert all(np.isfinite(v).all() for v in out.values()), out
