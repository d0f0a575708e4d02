"""GPU (-m gpu): the forms of rs_ehs and rs_ehs_round_histograms that tools/gen_emd.py and a production caller run -- every board of a round in one launch
(boards = NULL), hand lists long enough for a second trip of k_ehs's grid-stride loop, every bin count, the flop at its LDS limit, and the tool end to end -- bit for
bit against the numpy restatement tests/np_ehs.py.  No tolerance anywhere.  Every test prints its figures on a line that starts with EHS-ROUNDS (pytest -s)."""
import concurrent.futures
import json
import os
import subprocess
import sys
import time

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
ROYAL_DRAW = [32, 36, 40, 44]        # T J Q K of suit 0: the run-out 48 puts a royal flush on the board, every live pair then has v = 0.5 exactly
FLOP_PAIRED = [0, 1, 20]
FLOP_FIRST = [0, 1, 2]               # board number 0
FLOP_MIDDLE = [5, 22, 40]            # board number C(5, 1) + C(22, 2) + C(40, 3) = 5 + 231 + 9880: no digit is trivial; rainbow
FLOP_LAST = [49, 50, 51]             # board number 22 099
FLOP_BINS, TURN_BINS = 20, 30        # what the whole rounds run at: the reference's gen_emd(1, ..., 20) and its commented-out turn call
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_emd.py")


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


def report(name, **figures):
    print("EHS-ROUNDS %s: %s" % (name, ", ".join("%s %s" % (k.replace("_", " "), ("%.3f" % v) if isinstance(v, float) else v) for k, v in figures.items())))


def hands_of(board):
    """every hole pair of the board followed by the board: uint8 [n][2 + len(board)], in np_ehs.hole_pairs order"""
    pairs = ne.hole_pairs(board)
    return np.concatenate([pairs, np.tile(np.asarray(board), (len(pairs), 1))], axis=1).astype(np.uint8)


def relabel(cards, perm):
    return [4 * (int(c) >> 2) + perm[int(c) & 3] for c in cards]


def sentinel_buffer(table, indexer, n_bins):
    rows = indexer.size(1)
    out = ab.RoundHistograms(table, rows, n_bins, DeviceBuffer(table, rows * n_bins * 4))
    L.check(L.load().rs_dmemset(table._h, out.ptr, 0xCD, out.nbytes))
    return out


def words_of(out, first=0, count=None):
    return out.download(first, count).view(np.uint32)


def rows_of(out, idx):
    """the rows `idx` (with repeats) of a table on the device, as words"""
    u, inv = np.unique(idx, return_inverse=True)
    return out.gather(u).view(np.uint32)[inv]


def compare_board(got_rows, board, n_bins):
    """the rows of every hand of the board, in hands_of order, against the restatement -> cells compared"""
    pairs, want = ne.board_histograms(board, n_bins)
    assert got_rows.shape == want.shape and len(pairs) == (1176 if len(board) == 3 else 1128)
    bad = np.nonzero((got_rows != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, (board, len(bad), pairs[bad[:5]].tolist(), got_rows[bad[:2]].view(F32), want[bad[:2]])
    return want.size


def check_exact(words, n_compl):
    """every word is one of the n_compl + 1 a cell can hold and each row's counts add up to n_compl -> (sentinel words, words that are no cell value, rows whose sum is off)"""
    k = ne.counts_of_words(words, n_compl)
    return int((words == SENTINEL).sum()), int((k < 0).sum()), int((k.sum(axis=1, dtype=np.int64) != n_compl).sum())


# ---- A. the whole round, every board ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flop_round(table, flop_indexer):
    """boards = None at 20 bins into a sentinel-filled table, once: (the table on the device, its words on the host, read-only)"""
    out = sentinel_buffer(table, flop_indexer, FLOP_BINS)
    t0 = time.perf_counter()
    assert ab.round_histograms(table, flop_indexer, FLOP_BINS, out=out) is out
    t1 = time.perf_counter()
    words = words_of(out)
    words.setflags(write=False)
    report("flop_round fixture", boards=22100, rows=out.rows, bins=FLOP_BINS, sweep_s=t1 - t0, download_s=time.perf_counter() - t1)
    yield out, words
    out.buffer.free()


@pytest.fixture(scope="module")
def turn_round(table, turn_indexer):
    """boards = None at 30 bins into a sentinel-filled table (1.7 GB), once; it stays on the device"""
    out = sentinel_buffer(table, turn_indexer, TURN_BINS)
    t0 = time.perf_counter()
    ab.round_histograms(table, turn_indexer, TURN_BINS, out=out)
    report("turn_round fixture", boards=270725, rows=out.rows, bins=TURN_BINS, sweep_s=time.perf_counter() - t0)
    yield out
    out.buffer.free()


def test_flop_round_sampled_boards_equal_the_restatement(flop_round, flop_indexer):
    """After the full sweep -- every canonical row written by all its suit-isomorphic boards at once, each board decoded from its workgroup's number -- the rows of the
    first, a middle and the last board are the restatement's"""
    out, words = flop_round
    t0, cells = time.perf_counter(), 0
    for number, board in ((0, FLOP_FIRST), (10116, FLOP_MIDDLE), (22099, FLOP_LAST)):
        assert ne.board_by_number(3, number) == board
        idx = flop_indexer.get_index(hands_of(board)).astype(np.int64)
        cells += compare_board(words[idx], board, FLOP_BINS)
    report("flop sampled boards", boards=3, rows=3 * 1176, cells=cells, differ=0, wall_s=time.perf_counter() - t0)


def turn_samples():
    rng = np.random.Generator(np.random.PCG64(2024))
    numbers = [0, 270724] + [ne.board_number(b) for b in (TURN_PAIRED, TURN_MONOTONE, ROYAL_DRAW)] + rng.integers(0, 270725, size=3).tolist()
    return [(n, ne.board_by_number(4, n)) for n in numbers]


def test_turn_round_sampled_boards_equal_the_restatement(turn_round, turn_indexer):
    t0, cells = time.perf_counter(), 0
    samples = turn_samples()
    assert samples[0][1] == [0, 1, 2, 3] and samples[1][1] == [48, 49, 50, 51] and [b for _, b in samples[2:5]] == [TURN_PAIRED, TURN_MONOTONE, ROYAL_DRAW]
    assert len({n for n, _ in samples}) == 8
    for number, board in samples:
        idx = turn_indexer.get_index(hands_of(board)).astype(np.int64)
        cells += compare_board(rows_of(turn_round, idx), board, TURN_BINS)
    report("turn sampled boards", boards=[n for n, _ in samples], rows=8 * 1128, cells=cells, differ=0, wall_s=time.perf_counter() - t0)


def test_flop_round_every_row_is_exact(flop_round):
    """No word still holds the sentinel, every word is f32(k) / f32(1081) for a whole k, and the k of every row add up to 1081: fails on a lost or doubled LDS atomic, a
    carry between the two uint16 halves of a word, a row written from a board with a repeated card, a torn write"""
    out, words = flop_round
    t0 = time.perf_counter()
    assert words.shape == (1286792, FLOP_BINS)
    sentinels, strange, off = check_exact(words, 1081)
    report("flop every row", rows=len(words), cells=words.size, sentinel_words=sentinels, words_that_are_no_count=strange, rows_with_another_sum=off, wall_s=time.perf_counter() - t0)
    assert (sentinels, strange, off) == (0, 0, 0)


def test_turn_round_every_row_is_exact(turn_round):
    """the same over the 13 960 050 rows at 30 bins, downloaded in slices; the slices are checked on a few threads while the next one arrives"""
    t0 = time.perf_counter()
    step, totals, rows = 1 << 19, np.zeros(3, dtype=np.int64), 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        pending = []
        for first in range(0, turn_round.rows, step):
            x = words_of(turn_round, first, min(step, turn_round.rows - first))
            rows += len(x)
            pending.append(pool.submit(check_exact, x, 46))
            del x
            while len(pending) >= 8:
                totals += pending.pop(0).result()
        for f in pending:
            totals += f.result()
    assert rows == turn_round.rows == 13960050
    report("turn every row", rows=rows, cells=rows * TURN_BINS, sentinel_words=int(totals[0]), words_that_are_no_count=int(totals[1]), rows_with_another_sum=int(totals[2]),
           wall_s=time.perf_counter() - t0)
    assert totals.tolist() == [0, 0, 0]


def test_a_relabelled_flop_listed_alone_writes_what_the_round_holds(table, flop_round, flop_indexer):
    """Suit symmetry at full size: FLOP_MIDDLE with its suits permuted is another workgroup of the full sweep; listed alone it writes the same rows (the indexer's
    property) with the same bits as the table of the whole round holds there"""
    full, words = flop_round
    t0 = time.perf_counter()
    twin = relabel(FLOP_MIDDLE, [2, 0, 3, 1])
    assert sorted(twin) != sorted(FLOP_MIDDLE) and sorted(c >> 2 for c in twin) == sorted(c >> 2 for c in FLOP_MIDDLE)
    out = sentinel_buffer(table, flop_indexer, FLOP_BINS)
    ab.round_histograms(table, flop_indexer, FLOP_BINS, boards=[twin], out=out)
    x = words_of(out)
    out.buffer.free()
    idx = np.unique(flop_indexer.get_index(hands_of(twin)).astype(np.int64))
    assert (idx == np.unique(flop_indexer.get_index(hands_of(FLOP_MIDDLE)).astype(np.int64))).all()
    differ = int((x[idx] != words[idx]).any(axis=1).sum())
    x[idx] = SENTINEL
    report("flop relabelled board", board=twin, rows=len(idx), cells=len(idx) * FLOP_BINS, differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0
    assert x.min() == SENTINEL and x.max() == SENTINEL, "a row of no listed board was written"


def test_relabelled_turn_boards_listed_alone_write_what_the_round_holds(table, turn_round, turn_indexer):
    t0 = time.perf_counter()
    originals = [TURN_PAIRED, turn_samples()[5][1]]
    twins = [relabel(originals[0], [3, 2, 1, 0]), relabel(originals[1], [1, 2, 3, 0])[::-1]]      # a listed board need not be ascending
    out = ab.round_histograms(table, turn_indexer, TURN_BINS, boards=twins)                       # the other rows: zero
    differ = rows = 0
    for board, twin in zip(originals, twins):
        assert sorted(twin) != sorted(board)
        idx = np.unique(turn_indexer.get_index(hands_of(twin)).astype(np.int64))
        assert (idx == np.unique(turn_indexer.get_index(hands_of(board)).astype(np.int64))).all()
        differ += int((rows_of(out, idx) != rows_of(turn_round, idx)).any(axis=1).sum())
        rows += len(idx)
    out.buffer.free()
    report("turn relabelled boards", boards=twins, rows=rows, cells=rows * TURN_BINS, differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0


def shuffled_boards(nb, seed):
    every = ne.round_boards(nb)
    return every[np.random.Generator(np.random.PCG64(seed)).permutation(len(every))]


def test_flop_round_equals_every_board_listed(table, flop_round, flop_indexer):
    """boards = NULL against the listed path over the whole round: all 22 100 boards from the restatement's numbering, in a shuffled order"""
    full, words = flop_round
    t0 = time.perf_counter()
    boards = shuffled_boards(3, 31)
    assert boards.shape == (22100, 3)
    out = sentinel_buffer(table, flop_indexer, FLOP_BINS)
    t1 = time.perf_counter()
    ab.round_histograms(table, flop_indexer, FLOP_BINS, boards=boards, out=out)
    t2 = time.perf_counter()
    x = words_of(out)
    out.buffer.free()
    differ = int((x != words).sum())
    report("flop NULL against listed", boards=len(boards), rows=len(x), cells=x.size, differ=differ, listed_sweep_s=t2 - t1, wall_s=time.perf_counter() - t0)
    assert differ == 0


def test_turn_round_equals_every_board_listed(table, turn_indexer):
    """the same for the turn, at 2 bins: the bin count does not enter the decode of a board, and two tables of 112 MB are downloaded where 30 bins would need 2 x 1.7 GB.
    The 2-bin table is held to the exact-row rule as well"""
    t0 = time.perf_counter()
    boards = shuffled_boards(4, 32)
    assert boards.shape == (270725, 4)
    a, b = sentinel_buffer(table, turn_indexer, 2), sentinel_buffer(table, turn_indexer, 2)
    t1 = time.perf_counter()
    ab.round_histograms(table, turn_indexer, 2, out=a)
    t2 = time.perf_counter()
    ab.round_histograms(table, turn_indexer, 2, boards=boards, out=b)
    t3 = time.perf_counter()
    x, y = words_of(a), words_of(b)
    a.buffer.free()
    b.buffer.free()
    differ = int((x != y).sum())
    exact = check_exact(x, 46)
    report("turn NULL against listed", boards=len(boards), rows=len(x), cells=x.size, differ=differ, exact_row_rule=exact, null_sweep_s=t2 - t1, listed_sweep_s=t3 - t2,
           wall_s=time.perf_counter() - t0)
    assert differ == 0 and exact == (0, 0, 0)


# ---- B. long lists through rs_ehs: every workgroup of the capped grid takes a second trip ------------------------------------------------------------------------
def river_hands(board5):
    """all 1081 hands of a river board and their exact EHS through the rank-order form"""
    pairs, W, T = ne.river_counts_sorted(board5)
    hands = np.concatenate([pairs, np.tile(np.asarray(board5), (len(pairs), 1))], axis=1).astype(np.uint8)
    return hands, np.array([ne.ehs_value(k, 2 * ne.N_OPP) for k in 2 * W + T], dtype=F32)


def long_list(n_cards):
    """-> (hands, their EHS, hands a workgroup takes per trip): the hands the suite computes anyway, tiled past 65 536 workgroups' worth.  The period is no divisor of
    the stride, so the hand of a workgroup's second trip is another one than that of its first"""
    if n_cards == 7:
        base, want = zip(*(river_hands(b) for b in (BROADWAY, PAIRED, FOUR_FLUSH, RAINBOW)))
        base, want, reps, per = np.concatenate(base), np.concatenate(want), 61, 4
    else:
        board, reps, per = (TURN_PAIRED, 59, 1) if n_cards == 6 else (FLOP_MIDDLE, 56, 1)
        n_compl = 46 if n_cards == 6 else 1081
        pairs, k2 = ne.board_counts(board)
        assert ((k2 >= 0).sum(axis=1) == n_compl).all()
        base = hands_of(board)
        want = np.array([ne.ehs_value(int(k), 2 * ne.N_OPP * n_compl) for k in np.where(k2 >= 0, k2, 0).sum(axis=1)], dtype=F32)
    assert len(base) == {7: 4324, 6: 1128, 5: 1176}[n_cards] and (65536 * per) % len(base) != 0
    hands, want = np.tile(base, (reps, 1)), np.tile(want, reps)
    assert len(hands) == {7: 263764, 6: 66552, 5: 65856}[n_cards] and len(hands) > 65536 * per
    return hands, want, per


def run_ehs(table, hands):
    """rs_ehs through the C ABI into a sentinel-filled buffer that is longer than the list -> (return code, every word of the buffer, seconds)"""
    n, n_cards = hands.shape
    dc, _ = ab._card_rows(table, hands, n_cards)
    do = DeviceBuffer(table, (deal_pitch(n) + 64) * 4)
    L.check(L.load().rs_dmemset(table._h, do.ptr, 0xCD, do.nbytes))
    t0 = time.perf_counter()
    rc = L.load().rs_ehs(table._h, dc.ptr, n_cards, n, do.ptr)       # synchronises: it reads the error word back
    t = time.perf_counter() - t0
    return rc, do.download(np.uint32, do.nbytes // 4), t


@pytest.mark.parametrize("n_cards", [7, 6, 5])
def test_ehs_long_lists_take_the_second_trip(table, n_cards):
    t0 = time.perf_counter()
    hands, want, per = long_list(n_cards)
    n = len(hands)
    rc, got, t_good = run_ehs(table, hands)
    assert rc == L.OK
    differ = int((got[:n] != bits(want)).sum())
    assert differ == 0, np.nonzero(got[:n] != bits(want))[0][:10]
    assert (got[n:] == SENTINEL).all()
    # one bad hand in the second trip: reported, left alone, and every other hand is done
    p = 65536 * per + 301
    assert p < n and (p // per) - 65536 == 301 // per            # workgroup 75 (7 cards, its wave 1) or 301 comes back for it
    bad = hands.copy()
    bad[p, n_cards - 1] = bad[p, 0]
    rc, got, t_bad = run_ehs(table, bad)
    assert rc == L.ERR_INVALID and "repeats a card" in L.load().rs_last_error().decode()
    good = np.arange(n) != p
    assert got[p] == SENTINEL and (got[:n][good] == bits(want)[good]).all() and (got[n:] == SENTINEL).all()
    report("rs_ehs long list, %d cards" % n_cards, hands=n, differ=differ, launch_s=t_good, launch_with_a_bad_hand_s=t_bad, wall_s=time.perf_counter() - t0)


# ---- C. every bin count, and the flop at its LDS limit -----------------------------------------------------------------------------------------------------------
def written_rows(table, out):
    """the rows of a table on the device that are not all sentinel, found on the device: the L2 distance (rs_kmeans_predict, one center) of a row to the row of
    sentinels is sqrt(sum (x - s)^2), +0.0 if and only if every word is the sentinel -- s = -4.3e8 is finite, x - s is 0 for x = s alone and at least one step of s
    (32) otherwise, or inf / NaN.  Only the distances come to the host: 4 bytes per row in place of 4 n_bins"""
    center = np.full((1, out.n_bins), SENTINEL, dtype=np.uint32).view(F32)
    dm = DeviceBuffer(table, out.rows * 4)
    L.check(L.load().rs_kmeans_predict(table._h, ab.DIST_L2, out.ptr, out.rows, center.ctypes.data, 1, out.n_bins, None, dm.ptr))
    d = dm.download(F32, out.rows)
    dm.free()
    return np.nonzero(~(d == 0))[0]


@pytest.mark.parametrize("n_bins", range(1, ab.EHS_MAX_BINS + 1))
def test_turn_histograms_at_every_bin_count(table, turn_indexer, n_bins):
    """ROYAL_DRAW and TURN_PAIRED, listed, at all 64 bin counts: the binary search over the staged thresholds against get_bin's downward loop, on boards whose run-outs
    put values exactly on thresholds (test_ehs_cpu.py lists which).  The rows of the two boards are the restatement's; no other row of the table was written"""
    t0 = time.perf_counter()
    boards = [ROYAL_DRAW, TURN_PAIRED]
    out = sentinel_buffer(table, turn_indexer, n_bins)
    ab.round_histograms(table, turn_indexer, n_bins, boards=boards, out=out)
    cells, rows = 0, []
    for board in boards:
        idx = turn_indexer.get_index(hands_of(board)).astype(np.int64)
        cells += compare_board(rows_of(out, idx), board, n_bins)
        rows.append(idx)
    touched = np.unique(np.concatenate(rows))
    written = written_rows(table, out)
    assert np.array_equal(written, touched), "a row of no listed board was written"
    if n_bins <= 2:      # the device-side scan against the download it stands in for
        x = words_of(out)
        assert np.array_equal(np.nonzero((x != SENTINEL).any(axis=1))[0], written)
    out.buffer.free()
    report("turn at %d bins" % n_bins, rows=2 * 1128, cells=cells, differ=0, rows_written=len(written), wall_s=time.perf_counter() - t0)


def check_table(x, indexer, boards, n_bins):
    """check_rows of test_gpu_ehs.py on a downloaded table: the rows of every hand on `boards` are the restatement's, every other row still holds the sentinel"""
    touched = []
    for board in boards:
        idx = indexer.get_index(hands_of(board)).astype(np.int64)
        compare_board(x[idx], board, n_bins)
        touched.append(idx)
    x[np.unique(np.concatenate(touched))] = SENTINEL
    assert x.min() == SENTINEL and x.max() == SENTINEL, "a row of no listed board was written"


def listed_flop_sweep(table, flop_indexer, boards, n_bins):
    """through the C ABI, with nothing allocated or freed by the caller around the call -> (the table's words, device bytes held after minus before)"""
    lib = L.load()
    out = sentinel_buffer(table, flop_indexer, n_bins)
    db, n = ab._card_rows(table, boards, 3)
    before = lib.rs_device_held_bytes()
    L.check(lib.rs_ehs_round_histograms(table._h, flop_indexer._h, n_bins, db.ptr, n, out.ptr))
    held = lib.rs_device_held_bytes() - before
    x = words_of(out)
    out.buffer.free()
    return x, held


@pytest.mark.parametrize("n_bins", [1, 2, 21, 63, 64])
def test_flop_histograms_up_to_the_lds_limit(table, flop_indexer, n_bins):
    """The flop above 20 bins.  At 64 the workgroup declares (2048 + 1088 + 64 + 1176 * 64 / 2) * 4 = 163 328 of the 163 840 bytes of LDS a workgroup may have"""
    t0 = time.perf_counter()
    assert (2048 + 1088 + 64 + (1176 * 64 + 1) // 2) * 4 == 163328
    boards = [FLOP_PAIRED, FLOP_LAST]
    x, held = listed_flop_sweep(table, flop_indexer, boards, n_bins)
    assert held == 0
    check_table(x, flop_indexer, boards, n_bins)
    report("flop at %d bins" % n_bins, rows=2 * 1176, cells=2 * 1176 * n_bins, differ=0, wall_s=time.perf_counter() - t0)


def test_flop_at_20_bins_after_the_64_bin_launch(table, flop_indexer):
    """the LDS attribute set for the 64-bin launch stays on the kernel: the launches after it must be as right as the ones before"""
    t0 = time.perf_counter()
    x, held = listed_flop_sweep(table, flop_indexer, [FLOP_LAST], ab.EHS_MAX_BINS)
    assert held == 0 and (x != SENTINEL).any()
    x, held = listed_flop_sweep(table, flop_indexer, [FLOP_PAIRED, FLOP_LAST], FLOP_BINS)
    assert held == 0
    check_table(x, flop_indexer, [FLOP_PAIRED, FLOP_LAST], FLOP_BINS)
    report("flop at 20 bins after 64", rows=2 * 1176, cells=2 * 1176 * FLOP_BINS, differ=0, wall_s=time.perf_counter() - t0)


# ---- D. the tool, once, end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_gen_emd_gives_the_same_flop_bucket_file_twice(tmp_path, flop_indexer):
    t0 = time.perf_counter()
    files, lines, seconds = [tmp_path / "a.dat", tmp_path / "b.dat"], [], []
    for path in files:      # one fresh child at a time; the second only after the first came back clean
        t1 = time.perf_counter()
        r = subprocess.run([sys.executable, TOOL, "--round", "1", "--clusters", "64", "--bins", "20", "--seed", "7", "--out", str(path)], capture_output=True, text=True,
                           timeout=120)
        seconds.append(time.perf_counter() - t1)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = flop_indexer.size(1)
    assert rows == 1286792
    assert files[0].read_bytes() == files[1].read_bytes()
    for line in lines:
        assert line["rows"] == rows and line["count_sum"] == rows * 1081 and line["clusters"] == 64 and line["seed"] == 7
    assert lines[0]["xor"] == lines[1]["xor"] and lines[0]["inertia"] == lines[1]["inertia"]
    clusters = ab.read_cluster_file(str(files[0]))
    assert clusters.dtype == np.uint32 and clusters.shape == (rows,) and int(clusters.max()) < 64
    assert len(np.unique(clusters)) == lines[0]["used_clusters"] > 1
    # CardAbstraction reads it as the flop's bucket file
    mask = sum(1 << c for c in FLOP_MIDDLE)
    hole = ab.random_range(mask)
    card_abs = ab.CardAbstraction.init([hole, hole], mask, ab.FLOP, clusters)
    assert card_abs.index_size() == rows and 1 < card_abs.get_size(0) <= 64
    hands = np.concatenate([hole, np.tile(np.asarray(FLOP_MIDDLE, dtype=np.uint8), (len(hole), 1))], axis=1)
    dense = card_abs.get_cluster(hands, 0)
    file_cluster = clusters[flop_indexer.get_index(hands).astype(np.int64)]
    assert len(set(zip(dense.tolist(), file_cluster.tolist()))) == len(set(file_cluster.tolist())) == card_abs.get_size(0)
    # hands with bit-equal histograms (the restatement's, of the three flops the full sweep is sampled at) lie in one cluster, whichever rows they have
    by_histogram = {}
    for board in (FLOP_FIRST, FLOP_MIDDLE, FLOP_LAST):
        pairs, h = ne.board_histograms(board, FLOP_BINS)
        for row, hb in zip(flop_indexer.get_index(hands_of(board)).astype(np.int64).tolist(), bits(h)):
            by_histogram.setdefault(hb.tobytes(), set()).add(row)
    shared = [sorted(r) for r in by_histogram.values() if len(r) > 1]
    assert len(shared) >= 5
    split = [r for r in shared if len(set(clusters[r].tolist())) != 1]
    report("gen_emd twice", tool_runs_s=seconds, histograms_shared_by_several_rows=len(shared), rows_in_them=sum(len(r) for r in shared), split_between_clusters=len(split),
           used_clusters=lines[0]["used_clusters"], wall_s=time.perf_counter() - t0)
    assert not split, split[:3]
