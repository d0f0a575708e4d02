"""GPU (-m gpu): rake on the deal path -- rs_solver_create_deals_raked and rs_deal_trainer_set_rake.

Two yardsticks, both bit for bit on both table arrays and on the root utilities (the generated kernels are compiled with -ffp-contract=off and a raked leaf yields the f32
numbers a utility row would hold, so nothing is left to a tolerance):
  * oracle/np_walk.iterate_deals on tests/np_rake_deals.py's retyped tree and utility rows (pinned without rake by tests/test_rake_deals_cpu.py);
  * the device's own UNRAKED deal solver on the same retyped tree with RS_LEAF_UTIL buffers of those rows.
Shapes are the smallest that reach every path: 257 deals (ragged against 64 and 4) on 7 / 5 clusters, a sign row with -1, 0 and +1, rake (0.3, cap) with the cap on both
sides of the tree's pots (asserted).  The two-round tree adds round subtrees, boundaries, reach-down halves and lists, under every rs_kernel_forms choice.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import np_rake_deals as nrd
import rustsolver_amd as rs
from oracle import np_restate as npr
from oracle import np_walk as npw
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd import rake as raked
from test_rake_deals_cpu import RIVER_RAKE, TWO_ROUND, TWO_ROUND_RAKE, both_sides_of_the_cap, signs

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = {"i32": rs.I32, "f32": rs.F32, "f16": rs.F16}
FILL = {"i32": ((-3 * 10**7, 10**7), (0, 10**6)),   # a quarter of the regrets below the prune threshold of -10 000 000
         "f32": ((-10**6, 10**6), (0, 10**6)), "f16": ((-1000, 1000), (0, 1000))}
SCALE = {"i32": 100.0, "f32": 100.0, "f16": 0.5}
RIVER_BOARD = "4d5dAs3cKs"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: these tests need a real MI355X (there is no CPU fallback)")


def canon(x):
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    a, b = (got.reshape(-1), want.reshape(-1)) if want.dtype == np.int32 else (canon(got), canon(want))
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d/%d values differ, first at %d: %r vs %r" % (what, bad.size, b.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def table_as_numpy(table, tree):
    """{action index: (R, S)} as np_walk takes it: int32, or float32 holding the table's values"""
    out = {}
    for nd in tree.action_nodes():
        r, s = table.download_node(nd.index)
        out[nd.index] = (r.copy(), s.copy()) if r.dtype == np.int32 else (r.astype(F32), s.astype(F32))
    return out


def same_tables(table, tab, what):
    for idx, (R, S) in tab.items():
        r, s = table.download_node(idx)
        same(r, R, "%s: regrets of node %d" % (what, idx))
        same(s, S, "%s: strategy sums of node %d" % (what, idx))


class Case:
    """one tree, one batch of deals, one filled table per solver that is asked for"""

    def __init__(self, options, n_rounds, n_deals, seed, dtype):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.n_act, self.tree = rs.build_game_tree(options)
        self.retree, self.renodes = nrd.retyped_tree(self.tree), nrd.retyped_nodes(self.tree)
        self.sizes, self.n, self.seed, self.dtype = [(7, 5)] * n_rounds, n_deals, seed, dtype
        self.cidx = {(r, p): self.rng.integers(0, self.sizes[r][p], size=n_deals).astype(np.uint32) for r in range(n_rounds) for p in (0, 1)}
        self.sign = signs(self.rng, n_deals)
        self.flags = (self.rng.integers(0, 2, n_deals)).astype(np.uint8)
        assert 0 < self.flags.sum() < n_deals
        self.showdowns = [i for i, nd in enumerate(self.tree.nodes) if nd.kind == L.NODE_TERMINAL and nd.ttype != L.TERM_UNCONTESTED]

    def table(self, tree=None):
        t = rs.create_infosets(self.n_act, tree or self.tree, self.sizes, [1] * len(self.sizes), DTYPES[self.dtype])
        t.fill_random(self.seed, *FILL[self.dtype])
        return t

    def mode(self, prune):
        return rs.UPD_CLAMP_I64 | (rs.UPD_PRUNE if prune else 0)

    def raked_solver(self, table, rake, opp="sample", prune=False, forms=None, fuse=None, util_at=None):
        """rs_solver_create_deals_raked on the tree as it is: one sign row for every showdown / all-in terminal (util_at: {terminal: row} given as RS_LEAF_UTIL instead)"""
        dsign = rs.deal_buffer(table, self.n, self.sign)
        leaves = {i: (rs.LEAF_SIGN, dsign) for i in self.showdowns}
        for i, row in (util_at or {}).items():
            leaves[i] = (rs.LEAF_UTIL, rs.deal_buffer(table, self.n, row))
        return rs.MCCFRTrainer(self.tree, table, leaves, scale=SCALE[self.dtype], mode=self.mode(prune), fuse_subtrees=fuse, deals=self.cidx,
                               opp_mode=rs.OPP_SAMPLE if opp == "sample" else rs.OPP_FULL, sample_seed=self.seed, prune_deal=self.flags if prune else None, forms=forms, rake=rake)

    def util_solver(self, table, rake, opp="sample", prune=False, forms=None):
        """the unraked deal solver on the retyped tree: every terminal an RS_LEAF_UTIL buffer, one set per traverser"""
        lv = [{i: (rs.LEAF_UTIL, rs.deal_buffer(table, self.n, row)) for i, row in nrd.util_rows(self.tree, rake, self.sign, p).items()} for p in (0, 1)]
        return rs.MCCFRTrainer(self.retree, table, lv[0], leaves_p1=lv[1], scale=SCALE[self.dtype], mode=self.mode(prune), deals=self.cidx,
                               opp_mode=rs.OPP_SAMPLE if opp == "sample" else rs.OPP_FULL, sample_seed=self.seed, prune_deal=self.flags if prune else None, forms=forms)

    def numpy_sweep(self, tab, rake, player, k, opp="sample", prune=False, util_at=None):
        leaves = nrd.util_leaves(self.tree, rake, self.sign, player)
        for i, row in (util_at or {}).items():
            leaves[i] = ("util", np.asarray(row, dtype=F32))
        return npw.iterate_deals(self.renodes, tab, leaves, self.cidx, player, scale=SCALE[self.dtype], mode="clamp", prune=prune, prune_deal=self.flags if prune else None,
                                 dtype=self.dtype, opp=opp, seed=npr.sweep_seed(self.seed, k))

    def check(self, rake, opp="sample", prune=False, forms=None, numpy=True, device=True, iters=2, util_at=None):
        table = self.table()
        solver = self.raked_solver(table, rake, opp, prune, forms, util_at=util_at)
        tab = table_as_numpy(table, self.tree)
        other = self.table(self.retree) if device else None
        twin = self.util_solver(other, rake, opp, prune, forms) if device else None
        k = 0
        for it in range(iters):
            for player in (0, 1):
                got = solver.iterate(player, want_root_util=True)
                what = "%s %s it=%d p=%d" % (self.dtype, opp, it, player)
                if numpy:
                    same(got, self.numpy_sweep(tab, rake, player, k, opp, prune, util_at), "root utilities against numpy, " + what)
                if device:
                    same(got, twin.iterate(player, want_root_util=True), "root utilities against the util-leaf solver, " + what)
                k += 1
        if numpy:
            same_tables(table, tab, "against numpy")
        if device:
            same_tables(table, table_as_numpy(other, self.retree), "against the util-leaf solver")
        solver.destroy()
        if twin:
            twin.destroy()


# ---- the river tree ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,opp,prune", [("i32", "full", False), ("i32", "sample", False), ("i32", "sample", True), ("f32", "sample", False), ("f16", "sample", False)])
def test_raked_river_sweeps(dtype, opp, prune):
    case = Case(rs.Options(), 1, 257, 41, dtype)
    both_sides_of_the_cap(case.tree, RIVER_RAKE)
    case.check(RIVER_RAKE, opp=opp, prune=prune)


# ---- two rounds: round subtrees, boundaries, reach-down halves, lists -----------------------------------------------------------------------------------------------
FORMS = {
    "defaults": {},
    "deal_order": {"deal_order": rs.FORM_ON},
    "no_delta_rows": {"delta_rows": rs.FORM_OFF},
    "one_deal_per_thread": {"deals_per_thread": 1},
    "no_kept_records": {"kept_records": rs.FORM_OFF},
}


@pytest.mark.parametrize("dtype", ["i32", "f32"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_raked_two_round_sweeps(form, dtype):
    case = Case(rs.Options(**TWO_ROUND), 2, 300, 43, dtype)
    both_sides_of_the_cap(case.tree, TWO_ROUND_RAKE)
    case.check(TWO_ROUND_RAKE, forms=FORMS[form], device=False)


def test_raked_two_round_sweeps_against_the_util_leaf_solver():
    case = Case(rs.Options(**TWO_ROUND), 2, 300, 44, "i32")
    case.check(TWO_ROUND_RAKE, numpy=False)


# ---- a rake that is none ---------------------------------------------------------------------------------------------------------------------------------------------
def swept(case, solver, table):
    roots = [solver.iterate(p, want_root_util=True).copy() for p in (0, 1, 0, 1)]
    return roots, table_as_numpy(table, case.tree), [solver.n_launches(p) for p in (0, 1)]


@pytest.mark.parametrize("rake", ["NULL", (0.0, 0.0), (0.0, 5.0), (0.3, 0.0)])
def test_no_rake_is_the_unraked_solver(rake, monkeypatch):
    case = Case(rs.Options(**TWO_ROUND), 2, 300, 45, "i32")
    t0 = case.table()
    plain = case.raked_solver(t0, None)       # rake=None: rs_solver_create_deals itself
    want = swept(case, plain, t0)
    if rake == "NULL":                        # rs_solver_create_deals_raked with a NULL rake
        monkeypatch.setattr(raked, "arg", lambda r: (None, None))
        rake = (0.3, 30.0)
    t1 = case.table()
    solver = case.raked_solver(t1, rake)
    got = swept(case, solver, t1)
    assert got[2] == want[2]
    for a, b in zip(got[0], want[0]):
        same(a, b, "root utilities")
    for idx in want[1]:
        same(got[1][idx][0], want[1][idx][0], "regrets of node %d" % idx)
        same(got[1][idx][1], want[1][idx][1], "strategy sums of node %d" % idx)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_alone():
    case = Case(rs.Options(), 1, 257, 46, "i32")
    table = case.table()
    before = table.checksum()
    with pytest.raises(rs.RsError) as e:
        case.raked_solver(table, RIVER_RAKE, fuse=0)
    assert e.value.code == L.ERR_UNSUPPORTED
    for bad in ((-0.1, 5.0), (1.5, 5.0), (float("nan"), 5.0), (float("inf"), 5.0), (0.3, -1.0), (0.3, float("nan")), (0.3, 5.0, (1, 0)), (0.3, 5.0, (0, 7))):
        with pytest.raises(rs.RsError) as e:
            case.raked_solver(table, bad)
        assert e.value.code == L.ERR_INVALID, bad
    assert table.checksum() == before
    with pytest.raises(rs.RsError):            # lane solvers take no rake
        rs.MCCFRTrainer(case.tree, table, {}, rake=RIVER_RAKE)


def test_a_util_leaf_is_used_verbatim_under_a_rake():
    case = Case(rs.Options(), 1, 257, 47, "i32")
    at = case.showdowns[len(case.showdowns) // 2]
    row = (case.rng.uniform(-1, 1, case.n) * 500).astype(F32)
    case.check(RIVER_RAKE, device=False, util_at={at: row})


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_river_game():
    """about 12 combos per player on a river board, one cluster per hand"""
    mask = ab.card_mask(RIVER_BOARD)
    board = [c for c in range(52) if mask >> c & 1]
    rng = np.random.Generator(np.random.PCG64(93))
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.permutation(len(allh))[:12])], allh[np.sort(rng.permutation(len(allh))[:13])]]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    card_abs = [ab.CardAbstraction.init(ranges, mask, 2, None)]
    cids = [[card_abs[0].get_cluster(np.concatenate([ranges[p], np.tile(np.array(board, dtype=np.uint8), (len(ranges[p]), 1))], axis=1), p).reshape(1, -1) for p in (0, 1)]]
    return mask, board, ranges, tree, card_abs, cids


def replay(tr, tree, renodes, tab, rake, seed, k, dtype="i32"):
    """the trainer's live batch through the numpy yardstick, both traversers"""
    cidx = {(0, p): tr.clusters(0, p) for p in (0, 1)}
    sign = tr.signs()
    for player in (0, 1):
        npw.iterate_deals(renodes, tab, nrd.util_leaves(tree, rake, sign, player), cidx, player, scale=100.0, mode="clamp", dtype=dtype, opp="sample", seed=npr.sweep_seed(seed, k))
        k += 1
    return k


def test_raked_trainer_equals_the_yardstick():
    mask, board, ranges, tree, card_abs, cids = small_river_game()
    both_sides_of_the_cap(tree, RIVER_RAKE)
    renodes = nrd.retyped_nodes(tree)
    tr = rs.DealTrainer(tree, card_abs, ranges, mask, 257, seed=19, discount_interval=0, prune_threshold=None, rake=RIVER_RAKE)
    tab, k = table_as_numpy(tr.infosets, tree), 0
    for b in range(2):
        tr.train(1)
        k = replay(tr, tree, renodes, tab, RIVER_RAKE, 19, k)
        same_tables(tr.infosets, tab, "batch %d" % b)
    tr.status()
    with pytest.raises(rs.RsError, match="before the trainer's first batch") as e:
        tr.set_rake(None)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(rs.RsError) as e:       # refused before the handle is looked at: any non-NULL value stands for a communicator here
        tr.attach_comm(C.c_void_p(64))
    assert e.value.code == L.ERR_UNSUPPORTED
    # the unraked trainer of the same seed trains another game on the same cards
    plain = rs.DealTrainer(tree, card_abs, ranges, mask, 257, seed=19, discount_interval=0, prune_threshold=None)
    plain.train(2)
    assert (plain.cards() == tr.cards()).all()
    assert any(plain.infosets.download_node(i)[0].tobytes() != tab[i][0].tobytes() for i in tab)


def test_rake_and_weights_compose_in_either_order():
    mask, board, ranges, tree, card_abs, cids = small_river_game()
    renodes = nrd.retyped_nodes(tree)
    rng = np.random.Generator(np.random.PCG64(94))
    w = [2.0 ** -rng.uniform(0, 4, len(r)) for r in ranges]
    kw = dict(seed=23, discount_interval=0, prune_threshold=None)
    first = rs.DealTrainer(tree, card_abs, ranges, mask, 257, weights=w, rake=RIVER_RAKE, **kw)      # weights, then rake
    second = rs.DealTrainer(tree, card_abs, ranges, mask, 257, **kw)
    second.set_rake(RIVER_RAKE)
    second.set_weights(w)
    unweighted = rs.DealTrainer(tree, card_abs, ranges, mask, 257, rake=RIVER_RAKE, **kw)
    tab = table_as_numpy(first.infosets, tree)
    for tr in (first, second, unweighted):
        tr.train(1)
    assert (first.cards() == second.cards()).all() and not (first.cards() == unweighted.cards()).all()
    replay(first, tree, renodes, tab, RIVER_RAKE, 23, 0)
    same_tables(first.infosets, tab, "weights then rake")
    same_tables(second.infosets, tab, "rake then weights")


def test_raked_trainer_measures_the_game_it_trains():
    """best_response(), node_report() and train_full_width() of a raked trainer are the table's raked calls on the same game, bit for bit"""
    mask, board, ranges, tree, card_abs, cids = small_river_game()
    kw = dict(seed=29, discount_interval=0, prune_threshold=None, dtype=L.F32)
    tr, plain = rs.DealTrainer(tree, card_abs, ranges, mask, 257, rake=RIVER_RAKE, **kw), rs.DealTrainer(tree, card_abs, ranges, mask, 257, **kw)
    tr.train(2)
    for mode in (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED):
        got = tr.best_response(mode)
        want = tr.infosets.best_response_rounds(tree, board, ranges[0], ranges[1], cids, mode, rake=RIVER_RAKE)
        assert got.tobytes() == want.tobytes(), (hex(mode), got, want)
        assert got.tobytes() != tr.infosets.best_response_rounds(tree, board, ranges[0], ranges[1], cids, mode).tobytes()
    srt = L.BR_SORTED
    assert tr.exploitability() == raked.exploitability(tr.best_response(L.BR_MAX | srt), tr.best_response(L.BR_AVERAGE | srt))
    assert plain.exploitability() == float(plain.best_response(L.BR_MAX | srt).sum() / 2.0)
    ids = [i for i, nd in enumerate(tree.nodes) if nd.kind == L.NODE_ACTION][:3]
    for p in (0, 1):
        got = tr.node_report(p, ids)
        want = tr.infosets.node_report(tree, board, ranges[0], ranges[1], cids, p, ids, rake=RIVER_RAKE)
        for i in ids:
            for key in want[i]:
                assert got[i][key].tobytes() == want[i][key].tobytes(), (p, i, key)
    # full-width CFR: the raked trainer's own against RangeCFR(rake=) on a table that went the same way (the unraked trainer's, given the raked trainer's cells)
    for nd in tree.action_nodes():
        plain.infosets.upload_node(nd.index, *tr.infosets.download_node(nd.index))
    got = tr.train_full_width(3)
    solver = rs.RangeCFR(plain.infosets, tree, board, ranges[0], ranges[1], cids, rake=RIVER_RAKE)
    want = solver.train(3)
    assert got.tobytes() == want.tobytes(), (got, want)
    for nd in tree.action_nodes():
        a, b = tr.infosets.download_node(nd.index), plain.infosets.download_node(nd.index)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), nd.index
    solver.destroy()


# ---- it solves what it trains ------------------------------------------------------------------------------------------------------------------------------------------
SOLVE_RAKE = (0.5, float("inf"))
SOLVE_BATCHES = 4   # the shortest power of two at which the trained table's raked exploitability is below HALF the uniform table's on the MI355X: 48.17 uniform, 39.39 after 2
                    # batches, 17.10 after 4 (profiles/rake_deals.md)


def test_the_raked_trainer_solves_the_raked_game():
    """65 536 deals per batch on the small river game under a rake of half the pot: the average profile after training is less exploitable IN THE RAKED GAME than the
    untrained (uniform) table.  The same seed trained without rake is measured in the raked game too and printed, not asserted: general-sum CFR promises nothing about it."""
    mask, board, ranges, tree, card_abs, cids = small_river_game()
    kw = dict(seed=31, discount_interval=0, prune_threshold=None)
    tr = rs.DealTrainer(tree, card_abs, ranges, mask, 65536, rake=SOLVE_RAKE, **kw)
    e0 = tr.exploitability()
    tr.train(SOLVE_BATCHES)
    tr.status()
    e1 = tr.exploitability()
    plain = rs.DealTrainer(tree, card_abs, ranges, mask, 65536, **kw)
    plain.train(SOLVE_BATCHES)
    mx, av = (plain.infosets.best_response_rounds(tree, board, ranges[0], ranges[1], cids, m | L.BR_SORTED, rake=SOLVE_RAKE) for m in (L.BR_MAX, L.BR_AVERAGE))
    print("raked exploitability: uniform %.6f, %d batches raked %.6f, the same batches trained unraked %.6f" % (e0, SOLVE_BATCHES, e1, raked.exploitability(mx, av)))
    assert e1 < e0
