"""GPU (-m gpu): exact EHS (rs_ehs) and the round histograms (rs_ehs_round_histograms) through the C ABI, bit for bit against the numpy restatement tests/np_ehs.py."""
import os
import sys

import numpy as np
import pytest

import rustsolver_amd as rs
from rustsolver_amd import _lib as L
from rustsolver_amd import abstraction as ab
from rustsolver_amd.solver import DeviceBuffer, deal_pitch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ehs as ne  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 0xCDCDCDCD                # what rs_dmemset(0xCD) leaves in every word: no histogram value and no EHS has these bits
BROADWAY = [32, 37, 42, 47, 48]
PAIRED = [0, 1, 22, 35, 49]
FOUR_FLUSH = [0, 8, 20, 36, 45]
RAINBOW = [0, 10, 20, 25, 29]
TURN_PAIRED = [0, 1, 22, 35]         # 2s 2h 7d Tc
TURN_MONOTONE = [0, 12, 24, 40]      # four cards of suit 0
TURN_MONOTONE_TWIN = [2, 14, 26, 42]  # the same in suit 2
FLOP_RAINBOW = [1, 10, 20]
FLOP_PAIRED = [0, 1, 20]             # 2s 2h 7s: two-tone as well
FLOP_TRIPS = [0, 1, 2]               # three cards of one rank: the run-out that makes quads shares its rank with hole pairs


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture(scope="module")
def table():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


@pytest.fixture(scope="module")
def turn_indexer():
    return ab.HandIndexer([2, 4])


@pytest.fixture(scope="module")
def flop_indexer():
    return ab.HandIndexer([2, 3])


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def river_hands(board5):
    """all 1081 hands of a river board and their exact EHS through the rank-order form"""
    pairs, W, T = ne.river_counts_sorted(board5)
    hands = np.concatenate([pairs, np.tile(np.asarray(board5), (len(pairs), 1))], axis=1).astype(np.uint8)
    return hands, np.array([ne.ehs_value(k, 2 * ne.N_OPP) for k in 2 * W + T], dtype=F32)


@pytest.fixture(scope="module")
def river_reference():
    hands, want = zip(*(river_hands(b) for b in (BROADWAY, PAIRED, FOUR_FLUSH, RAINBOW)))
    return np.concatenate(hands), np.concatenate(want)


# ---- rs_ehs ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ehs_seven_cards_every_pair_of_four_boards(table, river_reference):
    hands, want = river_reference
    assert len(hands) == 4324
    got = ab.ehs(table, hands)
    assert (bits(got) == bits(want)).all(), np.nonzero(bits(got) != bits(want))[0][:10]
    # the direct enumeration of one hand (no rank order, no card removal) says the same
    assert got[17] == ne.ehs(hands[17])


@pytest.mark.parametrize("n", [1, 9, 65])   # one hand; one past a multiple of the four hands a workgroup takes; one past a wave's worth
def test_ehs_seven_cards_list_lengths(table, river_reference, n):
    hands, want = river_reference
    pick = np.arange(n) * 61 % len(hands)
    got = ab.ehs(table, hands[pick])
    assert (bits(got) == bits(want[pick])).all()


def test_ehs_six_cards_every_pair_of_a_turn_board(table):
    pairs, k2 = ne.board_counts(TURN_PAIRED)
    want = np.array([ne.ehs_value(int(row[row >= 0].sum()), 2 * ne.N_OPP * 46) for row in k2], dtype=F32)
    hands = np.concatenate([pairs, np.tile(np.asarray(TURN_PAIRED), (len(pairs), 1))], axis=1).astype(np.uint8)
    assert len(hands) == 1128
    got = ab.ehs(table, hands)
    assert (bits(got) == bits(want)).all(), np.nonzero(bits(got) != bits(want))[0][:10]
    assert got[5] == ne.ehs(hands[5])


def test_ehs_five_cards_on_one_flop(table):
    hands = np.array([[2, 30], [21, 22], [32, 44], [13, 27], [34, 47], [35, 46], [48, 49], [3, 51]], dtype=np.uint8)   # trips, sevens full, a flush draw, air, two twins
    hands = np.concatenate([hands, np.tile(np.asarray(FLOP_PAIRED, dtype=np.uint8), (len(hands), 1))], axis=1)
    want = np.array([ne.ehs(h) for h in hands], dtype=F32)
    got = ab.ehs(table, hands)
    assert (bits(got) == bits(want)).all(), (got, want)
    assert bits(got)[4] == bits(got)[5]            # suits 2 and 3 swapped, the flop holds neither
    assert got[1] > got[0] > got[3]


# ---- rs_ehs_round_histograms ------------------------------------------------------------------------------------------------------------------------------------
def sentinel_buffer(table, indexer, n_bins):
    rows = indexer.size(1)
    out = ab.RoundHistograms(table, rows, n_bins, DeviceBuffer(table, rows * n_bins * 4))
    L.check(L.load().rs_dmemset(table._h, out.ptr, 0xCD, out.nbytes))
    return out


def check_rows(out, indexer, boards, n_bins):
    """the rows of every hand on `boards` equal the restatement's; every other row still holds the sentinel.  -> {board: its rows' numbers}"""
    x = out.buffer.download(np.uint32, out.rows * n_bins).reshape(out.rows, n_bins)
    rows_of = {}
    for board in boards:
        pairs, want = ne.board_histograms(board, n_bins)
        hands = np.concatenate([pairs, np.tile(np.asarray(board), (len(pairs), 1))], axis=1).astype(np.uint8)
        idx = indexer.get_index(hands).astype(np.int64)
        assert len(idx) == (1176 if len(board) == 3 else 1128)
        bad = np.nonzero((x[idx] != bits(want)).any(axis=1))[0]
        assert len(bad) == 0, (board, hands[bad[:5]].tolist(), x[idx][bad[:2]].view(F32), want[bad[:2]])
        rows_of[tuple(board)] = idx
    touched = np.unique(np.concatenate(list(rows_of.values())))
    x[touched] = SENTINEL
    assert x.min() == SENTINEL and x.max() == SENTINEL, "a row of no listed board was written"
    return rows_of


@pytest.mark.parametrize("n_bins", [1, 2, 20, 30, 50, ab.EHS_MAX_BINS])
def test_turn_histograms_of_three_boards(table, turn_indexer, n_bins):
    boards = [TURN_PAIRED, TURN_MONOTONE, TURN_MONOTONE_TWIN]
    out = sentinel_buffer(table, turn_indexer, n_bins)
    assert ab.round_histograms(table, turn_indexer, n_bins, boards=boards, out=out) is out
    rows_of = check_rows(out, turn_indexer, boards, n_bins)
    a, b = rows_of[tuple(TURN_MONOTONE)], rows_of[tuple(TURN_MONOTONE_TWIN)]
    assert sorted(a.tolist()) == sorted(b.tolist()) and len(set(a.tolist())) < len(a)   # the twins' rows coincide, and a board's own suit-isomorphic pairs share rows
    out.buffer.free()


@pytest.mark.parametrize("flop", [FLOP_RAINBOW, FLOP_PAIRED, FLOP_TRIPS], ids=["rainbow", "paired", "trips"])
def test_flop_histograms_every_pair_of_a_flop(table, flop_indexer, flop):
    out = sentinel_buffer(table, flop_indexer, 20)
    ab.round_histograms(table, flop_indexer, 20, boards=[flop], out=out)
    check_rows(out, flop_indexer, [flop], 20)


def test_histogram_and_six_card_ehs_agree_through_the_restatement(table, turn_indexer):
    """Both device results of one turn board come out of the same integer counts of the restatement: the histogram from the bin of each run-out's 2 W + T, the 6-card
    EHS from their sum.  (No float identity between the two device results is asserted: the bins lose what the sum keeps.)"""
    pairs, k2 = ne.board_counts(TURN_MONOTONE)
    hands = np.concatenate([pairs, np.tile(np.asarray(TURN_MONOTONE), (len(pairs), 1))], axis=1).astype(np.uint8)
    lut = ne.bin_of_k2(20)
    count = np.zeros((len(pairs), 20), dtype=np.int64)
    for r in range(k2.shape[1]):
        live = k2[:, r] >= 0
        np.add.at(count, (np.nonzero(live)[0], lut[k2[live, r]]), 1)
    assert (count.sum(axis=1) == 46).all()
    out = ab.round_histograms(table, turn_indexer, 20, boards=[TURN_MONOTONE])
    idx = turn_indexer.get_index(hands).astype(np.int64)
    n = int(idx.max()) + 1
    got_h = out.buffer.download(np.float32, n * 20).reshape(n, 20)[idx]
    assert (bits(got_h) == bits(count.astype(F32) / F32(46))).all()
    got_e = ab.ehs(table, hands)
    want_e = np.array([ne.ehs_value(int(row[row >= 0].sum()), 2 * ne.N_OPP * 46) for row in k2], dtype=F32)
    assert (bits(got_e) == bits(want_e)).all()
    # what ties the two device results: every run-out's 2 W + T lies inside its bin, so the histogram's counts times the bins' ends bracket the sum the EHS holds.
    # Both integers are recovered exactly from the device's floats (counts <= 46, sums <= 91 080 < 2^24).
    got_count = np.rint(got_h.astype(np.float64) * 46).astype(np.int64)
    got_total = np.rint(got_e.astype(np.float64) * (2 * ne.N_OPP * 46)).astype(np.int64)
    assert (got_count == count).all() and (got_total == np.where(k2 >= 0, k2, 0).sum(axis=1)).all()
    ends = [np.nonzero(lut == b)[0] for b in range(20)]
    lo = np.array([e.min() if len(e) else 0 for e in ends], dtype=np.int64)
    hi = np.array([e.max() if len(e) else 0 for e in ends], dtype=np.int64)
    assert ((got_count * lo).sum(axis=1) <= got_total).all() and (got_total <= (got_count * hi).sum(axis=1)).all()
    out.buffer.free()


# ---- refusals and bad cards ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(table, flop_indexer):
    lib = L.load()
    rows = flop_indexer.size(1)
    out = DeviceBuffer(table, rows * (ab.EHS_MAX_BINS + 1) * 4)      # room for whatever a call that should have been refused might write
    L.check(lib.rs_dmemset(table._h, out.ptr, 0xCD, out.nbytes))
    boards, n = ab._card_rows(table, [FLOP_RAINBOW], 3)
    cards, _ = ab._card_rows(table, [[48, 49] + RAINBOW], 7)
    preflop, river, three = ab.HandIndexer([2]), ab.HandIndexer([2, 5]), ab.HandIndexer([2, 3, 1])
    before = lib.rs_device_held_bytes()                               # nothing is allocated either
    for ix in (preflop, river, three):
        assert lib.rs_ehs_round_histograms(table._h, ix._h, 20, boards.ptr, n, out.ptr) == L.ERR_INVALID
    for n_bins in (0, -3, ab.EHS_MAX_BINS + 1):
        assert lib.rs_ehs_round_histograms(table._h, flop_indexer._h, n_bins, boards.ptr, n, out.ptr) == L.ERR_INVALID
    assert lib.rs_ehs_round_histograms(table._h, flop_indexer._h, 20, boards.ptr, n, None) == L.ERR_INVALID
    assert lib.rs_ehs_round_histograms(table._h, flop_indexer._h, 20, None, 0, None) == L.ERR_INVALID      # every board, nowhere to write
    for n_cards in (4, 8, 2, 0):
        assert lib.rs_ehs(table._h, cards.ptr, n_cards, 1, out.ptr) == L.ERR_INVALID
    assert lib.rs_ehs(table._h, cards.ptr, 7, 1, None) == L.ERR_INVALID
    assert "rs_ehs" in lib.rs_last_error().decode()
    assert lib.rs_device_held_bytes() == before
    x = out.download(np.uint32, out.nbytes // 4)
    assert x.min() == SENTINEL and x.max() == SENTINEL
    # nothing to do is not an error
    assert lib.rs_ehs(table._h, None, 7, 0, None) == L.OK
    assert lib.rs_ehs_round_histograms(table._h, flop_indexer._h, 20, boards.ptr, 0, None) == L.OK


def test_bad_cards_are_reported_and_fault_nothing(table, river_reference, turn_indexer):
    hands, want = river_reference
    lst = hands[:9].copy()
    lst[2, 6] = lst[2, 0]          # a repeated card
    lst[5, 1] = 52                 # no card
    lst[7, 3] = 255
    dc, n = ab._card_rows(table, lst, 7)
    do = DeviceBuffer(table, deal_pitch(n) * 4)
    L.check(L.load().rs_dmemset(table._h, do.ptr, 0xCD, do.nbytes))
    with pytest.raises(rs.RsError) as e:
        L.check(L.load().rs_ehs(table._h, dc.ptr, 7, n, do.ptr))
    assert e.value.code == L.ERR_INVALID and "repeats a card" in str(e.value)
    got = do.download(np.uint32, n)
    good = np.array([i not in (2, 5, 7) for i in range(n)])
    assert (got[good] == bits(want[:9])[good]).all() and (got[~good] == SENTINEL).all()
    with pytest.raises(rs.RsError):
        ab.ehs(table, [48, 48, 0, 10, 20])
    # a listed board that repeats a card: reported, skipped; the board beside it is done
    out = ab.round_histograms(table, turn_indexer, 2, boards=[TURN_PAIRED])
    ref = out.download().copy()
    out.buffer.zero()
    with pytest.raises(rs.RsError) as e:
        ab.round_histograms(table, turn_indexer, 2, boards=[[7, 9, 7, 30], TURN_PAIRED, [1, 2, 3, 64]], out=out)
    assert e.value.code == L.ERR_INVALID
    assert (bits(out.download()) == bits(ref)).all()
    # ... and the calls after it are clean
    assert ab.ehs(table, hands[0]) == want[0]
    out.buffer.free()


# ---- into the k-means without a trip through the host ----------------------------------------------------------------------------------------------------------------
def test_kmeans_from_device_predicts_like_an_upload(table, turn_indexer):
    boards = [TURN_PAIRED, TURN_MONOTONE, TURN_MONOTONE_TWIN]
    out = ab.round_histograms(table, turn_indexer, 20, boards=boards)      # rows of other hands: zero, the empty histogram
    idx = np.unique(np.concatenate([turn_indexer.get_index(np.concatenate([p, np.tile(np.asarray(b), (len(p), 1))], axis=1).astype(np.uint8))
                                    for b in boards for p in [ne.hole_pairs(b)]])).astype(np.int64)
    rows = np.stack([ne.board_histograms(b, 20)[1] for b in boards]).reshape(-1, 20)
    rng = np.random.Generator(np.random.PCG64(5))
    centers = rows[rng.choice(len(rows), size=12, replace=False)]
    n = int(idx.max()) + 1
    km = ab.Kmeans.from_device(table, out, n, 20)
    cl, md = km.predict(centers)
    host = out.buffer.download(np.float32, n * 20).reshape(n, 20)[idx]
    cl2, md2 = ab.Kmeans(table, host).predict(centers)
    assert (cl[idx] == cl2).all() and (bits(md[idx]) == bits(md2)).all()
    assert len(set(cl2.tolist())) > 3
    with pytest.raises(ValueError):
        ab.Kmeans.from_device(table, out, out.rows + 1, 20)
    out.buffer.free()
