"""GPU (-m gpu): weighted dealing on the device (rs_deals_sample_weighted, rs_deal_trainer_set_weights) against the restatement in plain Python integers
(tests/np_weighted_deals.py), byte for byte: both distributions on boards of 3, 4 and 5 cards, deal numbers, the exact fallback, the law case whose statistics
tests/test_weighted_deals_cpu.py checks, one-hand and 1326-hand ranges, duplicate combos, give-ups and refusals; then the whole trainer against the CPU oracle with the
oracle's dealer replaced by the restatement, and the trainer's best response and node report against the table's weighted calls with weights (double)q."""
import functools

import numpy as np
import pytest

import np_weighted_deals as nwd
import rustsolver_amd as rs
import test_gpu_cards as tg
from oracle import np_restate as npr
from oracle import orc
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer, deal_pitch
from test_np_br_cpu import ATOL, RTOL
from test_weighted_deals_cpu import FALLBACK, LAW

pytestmark = pytest.mark.gpu
RIVER_BOARD = "4d5dAs3cKs"


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture(scope="module")
def table():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


def restated(seed, first, mask, h0, h1, w0, w1, deal, n, **kw):
    return nwd.generate_hands(seed, first, mask, h0, h1, None if w0 is None else nwd.quanta(w0), None if w1 is None else nwd.quanta(w1), deal, n, **kw)


@pytest.mark.parametrize("deal", nwd.DEALS)
@pytest.mark.parametrize("n_board", [3, 4, 5])
def test_device_sampler_equals_the_restatement(table, n_board, deal):
    """the ranges of test_device_deal_sampler_equals_oracle (300 and 7 hands), weights 2^-U(0, 20)"""
    rng = np.random.Generator(np.random.PCG64(70 + n_board))
    mask = sum(1 << int(c) for c in rng.permutation(52)[:n_board])
    allh = ab.random_range(mask)
    h0, h1 = allh[rng.permutation(len(allh))[:300]], allh[rng.permutation(len(allh))[:7]]
    w0, w1 = 2.0 ** -rng.uniform(0, 20, 300), 2.0 ** -rng.uniform(0, 20, 7)
    n = 5000
    stats = {}
    want = restated(1234, 1000, mask, h0, h1, w0, w1, deal, n, stats=stats)
    got = ab.sample_deals(table, 1234, 1000, mask, [h0, h1], n, weights=(w0, w1), deal=deal)
    print(n_board, deal, stats)
    assert got.shape == (9, n) and got.tobytes() == want.tobytes()
    assert (ab.sample_deals(table, 1234, 1500, mask, [h0, h1], 100, weights=(w0, w1), deal=deal) == want[:, 500:600]).all()   # deal numbers, not batch positions
    assert all(len(set(col.tolist())) == 9 for col in got.T)
    # one player's weights alone, and the other distribution, deal other cards
    assert (ab.sample_deals(table, 1234, 1000, mask, [h0, h1], 200, weights=(w0, None), deal=deal) == restated(1234, 1000, mask, h0, h1, w0, None, deal, 200)).all()
    other = "joint" if deal == "sequential" else "sequential"
    assert not (ab.sample_deals(table, 1234, 1000, mask, [h0, h1], 200, weights=(w0, w1), deal=other) == want[:, :200]).all()


def test_the_exact_fallback_on_the_device(table):
    mask, h0, w0, h1, w1, seed, n = FALLBACK
    stats = {}
    want = restated(seed, 0, mask, h0, h1, w0, w1, "sequential", n, stats=stats)
    assert stats["fallbacks"] >= 1 and stats["gave_up"] == 0
    got = ab.sample_deals(table, seed, 0, mask, [h0, h1], n, weights=(w0, w1), deal="sequential")   # raises unless the error word is 0
    assert got.tobytes() == want.tobytes()
    # without player 1's third hand some deals do not exist: bit 2, and the cards the device leaves are the restatement's (dealt columns and filled ones)
    stats = {}
    want = restated(seed, 0, mask, h0, h1[:2], w0, w1[:2], "sequential", n, stats=stats, give_up="fill")
    assert stats["gave_up"] > 0
    cards, err = raw_sample(table, seed, 0, mask, h0, h1[:2], n, ab.DealWeights(table, (w0, w1[:2]), (3, 2), "sequential"))
    assert err == 4 and cards.tobytes() == want.tobytes()


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_the_law_case_on_the_device(table, deal):
    """the 65 536 deals whose counts tests/test_weighted_deals_cpu.py holds to the law"""
    mask, h0, w0, h1, w1, seed, n = LAW
    want = restated(seed, 0, mask, h0, h1, w0, w1, deal, n)
    assert ab.sample_deals(table, seed, 0, mask, [h0, h1], n, weights=(w0, w1), deal=deal).tobytes() == want.tobytes()


def raw_sample(table, seed, first, mask, h0, h1, n, dw):
    """rs_deals_sample_weighted as it is -> (cards [9][n], error word); dw: a DealWeights or None"""
    h0, h1 = (np.ascontiguousarray(h, dtype=np.uint8).reshape(-1, 2) for h in (h0, h1))
    d0, d1 = DeviceBuffer.from_numpy(table, h0), DeviceBuffer.from_numpy(table, h1)
    pitch = deal_pitch(n)
    dc, de = DeviceBuffer(table, 9 * pitch), DeviceBuffer(table, 4)
    dc.zero()
    de.zero()
    L.check(L.load().rs_deals_sample_weighted(table._h, seed, first, mask, d0.ptr, len(h0), d1.ptr, len(h1), None if dw is None else dw._h, n, dc.ptr, de.ptr))
    table.sync()
    return dc.download(np.uint8, 9 * pitch).reshape(9, pitch)[:, :n], int(de.download(np.uint32, 1)[0])


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_one_hand_and_every_hand(table, deal):
    """the LDS rows at their smallest and at 1326 hands each (every combo of the deck: the ones that hold a board card never fit); more than one workgroup.  The
    deals a one-hand range cannot take part in give up, on the device as in the restatement"""
    rng = np.random.Generator(np.random.PCG64(12))
    mask = ab.card_mask("7h8hQc")
    every = np.array([(a, b) for a in range(52) for b in range(a + 1, 52)], dtype=np.uint8)
    assert len(every) == 1326
    w = 2.0 ** -rng.uniform(0, 12, 1326)
    free = [tuple(h) for h in every.tolist() if not nwd.combo(h) & mask]
    one = [free[500]]
    two = [next(h for h in free if not nwd.combo(h) & nwd.combo(one[0]))]
    for h0, w0, h1, w1, n in ((every, w, every, w[::-1].copy(), 3000), (every, w, one, [0.25], 700), (one, None, every, w, 700), (one, [3.0], two, None, 300)):
        stats = {}
        want = restated(5, 10, mask, h0, h1, w0, w1, deal, n, stats=stats, give_up="fill")       # a run-out (or the other player) that takes a card of the one hand: no deal
        cards, err = raw_sample(table, 5, 10, mask, h0, h1, n, ab.DealWeights(table, (w0, w1), (len(h0), len(h1)), deal))
        print(deal, len(h0), len(h1), stats)
        assert cards.tobytes() == want.tobytes() and err == (4 if stats["gave_up"] else 0) and stats["gave_up"] < n // 2


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_duplicate_combos_and_unit_weights(table, deal):
    rng = np.random.Generator(np.random.PCG64(13))
    mask = ab.card_mask("7h8hQc2d")
    allh = ab.random_range(mask)
    h0 = allh[rng.integers(0, 12, 40)]          # 12 distinct hands listed 40 times
    h1 = allh[rng.permutation(len(allh))[:25]]
    w0 = rng.integers(1, 9, 40) / 4.0
    want = restated(8, 0, mask, h0, h1, w0, None, deal, 1500)
    assert ab.sample_deals(table, 8, 0, mask, [h0, h1], 1500, weights=(w0, None), deal=deal).tobytes() == want.tobytes()
    want = restated(8, 0, mask, h0, h1, None, None, deal, 1500)
    assert ab.sample_deals(table, 8, 0, mask, [h0, h1], 1500, weights=(None, None), deal=deal).tobytes() == want.tobytes()


def test_no_weights_object_is_the_unweighted_sampler(table):
    rng = np.random.Generator(np.random.PCG64(14))
    mask = ab.card_mask("7h8hQc")
    allh = ab.random_range(mask)
    h0, h1 = allh[rng.permutation(len(allh))[:300]], allh[rng.permutation(len(allh))[:7]]
    cards, err = raw_sample(table, 1234, 1000, mask, h0, h1, 3000, None)
    assert err == 0 and cards.tobytes() == ab.sample_deals(table, 1234, 1000, mask, [h0, h1], 3000).tobytes() == orc.generate_hands(1234, 1000, mask, h0, h1, 3000).tobytes()


def test_give_ups_and_refusals(table):
    for deal in nwd.DEALS:
        with pytest.raises(RuntimeError, match="error word 4"):
            ab.sample_deals(table, 3, 0, 0b111, [[(10, 11)], [(11, 12)]], 64, weights=(None, None), deal=deal)
        cards, err = raw_sample(table, 3, 0, 0b111, [(10, 11)], [(11, 12)], 64, ab.DealWeights(table, (None, None), (1, 1), deal))
        assert err == 4 and (cards == np.arange(9, dtype=np.uint8)[:, None]).all()      # the lowest nine free cards, as rs_deals_sample leaves them
        with pytest.raises(rs.RsError):
            ab.sample_deals(table, 3, 0, 0b11, [[(10, 11)], [(12, 13)]], 64, weights=(None, None), deal=deal)      # invalid board mask
    dw = ab.DealWeights(table, (None, None), (5, 5))
    allh = ab.random_range(0b111)
    for n0, n1 in ((6, 5), (5, 4), (1, 1)):
        with pytest.raises(rs.RsError, match="hands"):
            ab.sample_deals(table, 3, 0, 0b111, [allh[:n0], allh[:n1]], 64, weights=dw)
    host_only = ab.DealWeights(None, (None, None), (5, 5))
    with pytest.raises(rs.RsError, match="device"):
        ab.sample_deals(table, 3, 0, 0b111, [allh[:5], allh[:5]], 64, weights=host_only)
    assert ab.sample_deals(table, 3, 0, 0b111, [allh[::200][:5], allh[100::200][:5]], 64, weights=dw).shape == (9, 64)
    assert dw.quanta(0).tolist() == [1 << 32] * 5


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
def weighted_oracle_batch(ctx, w, deal):
    """test_gpu_cards.oracle_batch with orc.generate_hands replaced by the restatement"""
    q = [nwd.quanta(x) for x in w]
    kept = orc.generate_hands
    orc.generate_hands = lambda seed, first, mask, h0, h1, n: nwd.generate_hands(seed, first, mask, h0, h1, q[0], q[1], deal, n)
    try:
        return tg.oracle_batch(ctx)
    finally:
        orc.generate_hands = kept


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("deal", nwd.DEALS)
def test_weighted_trainer_equals_the_oracle_on_the_river(deal, prefetch):
    """the river game of test_deal_trainer_reference_as_coded (3000 deals per batch, 5 batches, ticks on), weights 2^-U(0, 6)"""
    mask = ab.card_mask(RIVER_BOARD)
    hands = ab.random_range(mask)
    rng = np.random.Generator(np.random.PCG64(21))
    w = [2.0 ** -rng.uniform(0, 6, len(hands)) for _ in (0, 1)]
    ctx = tg.load_trainer_pair(rs.default_flop(), orc.options_default_river(), mask, [hands, hands], 1, 3000, seed=11, interval=4000, cap=13000, weights=w, deal=deal,
                               prefetch=prefetch)
    for b in range(5):
        ctx["tr"].train(1)
        cards = weighted_oracle_batch(ctx, w, deal)
        assert (ctx["tr"].cards() == cards).all()
        for p in (0, 1):
            assert (ctx["tr"].clusters(0, p) == ctx["cidx"][(0, p)]).all()
        assert (ctx["tr"].signs() == ctx["sign"]).all()
    ctx["tr"].status()
    assert ctx["tr"].iterations == 15000 == ctx["t"]
    tg.compare_trainer_tables(ctx)
    with pytest.raises(rs.RsError, match="before the trainer's first batch"):
        ctx["tr"].set_weights(w, deal)
    with pytest.raises(rs.RsError, match="before the trainer's first batch"):
        ctx["tr"].set_weights(None)
    # the weights mattered: the unweighted oracle deals other cards
    assert not (orc.generate_hands(11, 12000, mask, hands, hands, 3000) == cards).all()


@functools.lru_cache(maxsize=None)
def flop_game():
    rng = np.random.Generator(np.random.PCG64(77))
    mask = ab.card_mask("7h8hQc")
    allh = ab.random_range(mask)
    ranges = [allh[rng.permutation(len(allh))[:40]], allh[rng.permutation(len(allh))[:55]]]
    files = [rng.integers(0, 37, size=1286792, dtype=np.uint32), rng.integers(0, 61, size=13960050, dtype=np.uint32), None]
    w = [2.0 ** -rng.uniform(0, 6, len(r)) for r in ranges]
    return mask, ranges, files, w


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("deal", nwd.DEALS)
def test_weighted_trainer_equals_the_oracle_on_three_streets(deal, prefetch):
    """the flop game of test_deal_trainer_three_streets_from_a_flop_with_bucket_files at 64 deals per batch"""
    mask, ranges, files, w = flop_game()
    ctx = tg.load_trainer_pair(rs.three_street_options(), orc.options_three_street(), mask, ranges, 3, 64, seed=5, interval=100, cap=10**9, bucket_files=files, weights=w,
                               deal=deal, prefetch=prefetch)
    for b in range(5):
        ctx["tr"].train(1)
        cards = weighted_oracle_batch(ctx, w, deal)
        assert (ctx["tr"].cards() == cards).all()
        for r in range(3):
            for p in (0, 1):
                assert (ctx["tr"].clusters(r, p) == ctx["cidx"][(r, p)]).all()
        assert (ctx["tr"].signs() == ctx["sign"]).all()
    ctx["tr"].status()
    tg.compare_trainer_tables(ctx)


def test_trainer_refuses_bad_weights():
    mask = ab.card_mask(RIVER_BOARD)
    hands = ab.random_range(mask)[:30]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    card_abs = [ab.CardAbstraction.init([hands, hands], mask, 2, None)]
    w = np.ones(30)
    for bad in (0.0,):
        x = w.copy()
        x[3] = bad
        with pytest.raises(ValueError, match="drop it"):
            rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, weights=(x, None))
    for bad in (-1.0, np.nan, np.inf, 2.0**-40):
        x = w.copy()
        x[3] = bad
        with pytest.raises(rs.RsError):
            rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, weights=(None, x))
    with pytest.raises(ValueError):
        rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, weights=(w[:-1], None))
    with pytest.raises(KeyError):
        rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, deal="neither")
    # set and taken back before the first batch: the unweighted trainer's cards
    tr = rs.DealTrainer(tree, card_abs, [hands, hands], mask, 64, seed=4, weights=(w * 0.5, None), deal="joint")
    tr.set_weights(None)
    tr.train(1)
    assert (tr.cards() == orc.generate_hands(4, 0, mask, hands, hands, 64)).all()


# the oracle's table of the game below, measured on the CPU by oracle/np_br.py on tests/np_weighted.py's WeightedGame with weights (double)q: exploitability (half the sum
# of the two best-response values, chips per deal) of the zero table and after 5 batches of 3000 deals -- the batch count was picked there: 1 batch leaves every average
# strategy uniform (81.07), 2 batches 98.64, 3 batches 37.05
CPU_EXPLOITABILITY = {"sequential": (81.06869055857582, 20.762085832635954), "joint": (81.06049978242925, 19.942426529660263)}


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_trainer_measures_the_game_it_deals(deal):
    """trainer.best_response() and node_report() are the table's weighted calls with weights (double)q and the trainer's distribution, bit for bit; training lowers the
    weighted exploitability"""
    mask = ab.card_mask(RIVER_BOARD)
    board = [c for c in range(52) if mask >> c & 1]
    rng = np.random.Generator(np.random.PCG64(91))
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.permutation(len(allh))[:60])], allh[np.sort(rng.permutation(len(allh))[:70])]]
    w = [2.0 ** -rng.uniform(0, 4, n) for n in (60, 70)]
    q = [np.array(nwd.quanta(x), dtype=np.float64) for x in w]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    card_abs = [ab.CardAbstraction.init(ranges, mask, 2, None)]
    cids = [[card_abs[0].get_cluster(np.concatenate([ranges[p], np.tile(np.array(board, dtype=np.uint8), (len(ranges[p]), 1))], axis=1), p).reshape(1, -1) for p in (0, 1)]]
    tr = rs.DealTrainer(tree, card_abs, ranges, mask, 3000, seed=11, discount_interval=4000, discount_cap=13000, weights=w, deal=deal)
    e0 = tr.best_response(L.BR_MAX).sum() / 2
    plain = rs.DealTrainer(tree, card_abs, ranges, mask, 3000, seed=11, discount_interval=4000, discount_cap=13000)
    assert plain.best_response(L.BR_MAX).sum() / 2 != e0     # the unweighted game is another game
    plain.destroy()
    tr.train(5)
    tr.status()
    for mode in (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED, L.BR_MAX | L.BR_REAL | L.BR_SORTED):
        got = tr.best_response(mode)
        want = tr.infosets.best_response_rounds(tree, board, ranges[0], ranges[1], cids, mode, weights=(q[0], q[1]), deal=deal)
        assert got.tobytes() == want.tobytes(), (deal, hex(mode), got, want)
        if mode & L.BR_AVERAGE:
            assert abs(got.sum()) < 1e-9
    ids = [i for i, nd in enumerate(npr.build_tree()[0]) if nd["kind"] == "action"][:3]     # tree node ids; build_tree's defaults are default_flop()
    for p in (0, 1):
        got = tr.node_report(p, ids)
        want = tr.infosets.node_report(tree, board, ranges[0], ranges[1], cids, p, ids, weights=(q[0], q[1]), deal=deal)
        for i in ids:
            for key in want[i]:
                assert got[i][key].tobytes() == want[i][key].tobytes(), (deal, p, i, key)
    e5 = tr.best_response(L.BR_MAX).sum() / 2
    print(deal, "exploitability: zero table %.6f, after 5 batches %.6f" % (e0, e5))
    assert e5 < e0
    assert np.allclose([e0, e5], CPU_EXPLOITABILITY[deal], rtol=RTOL, atol=ATOL), (e0, e5)


@pytest.mark.parametrize("deal", nwd.DEALS)
def test_trainer_full_width_trains_the_game_it_deals(deal):
    """train_full_width() of a weighted F32 trainer is RangeCFR with weights (double)q on a table of the same shape, bit for bit: values and every cell"""
    mask = ab.card_mask(RIVER_BOARD)
    board = [c for c in range(52) if mask >> c & 1]
    rng = np.random.Generator(np.random.PCG64(92))
    allh = ab.random_range(mask)
    ranges = [allh[np.sort(rng.permutation(len(allh))[:30])], allh[np.sort(rng.permutation(len(allh))[:35])]]
    w = [2.0 ** -rng.uniform(0, 4, n) for n in (30, 35)]
    q = [np.array(nwd.quanta(x), dtype=np.float64) for x in w]
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    card_abs = [ab.CardAbstraction.init(ranges, mask, 2, None)]
    cids = [[card_abs[0].get_cluster(np.concatenate([ranges[p], np.tile(np.array(board, dtype=np.uint8), (len(ranges[p]), 1))], axis=1), p).reshape(1, -1) for p in (0, 1)]]
    kw = dict(seed=11, discount_interval=0, prune_threshold=None, dtype=L.F32)
    weighted, plain = rs.DealTrainer(tree, card_abs, ranges, mask, 256, weights=w, deal=deal, **kw), rs.DealTrainer(tree, card_abs, ranges, mask, 256, **kw)
    got = weighted.train_full_width(3)
    solver = rs.RangeCFR(plain.infosets, tree, board, ranges[0], ranges[1], cids, weights=(q[0], q[1]), deal=deal)
    want = solver.train(3)
    assert got.tobytes() == want.tobytes(), (deal, got, want)
    for nd in tree.action_nodes():
        a, b = weighted.infosets.download_node(nd.index), plain.infosets.download_node(nd.index)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), nd.index
    assert plain.train_full_width(3).tobytes() != got.tobytes()      # three more iterations of the UNWEIGHTED game on the other table: another game, other values
    solver.destroy()
