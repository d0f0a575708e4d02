"""GPU (-m gpu): rs_ochs_round_features and rs_ehs_preflop_counts -- listed boards of every street, the whole river and turn rounds, the refusals, the preflop
counts against a fold of the pinned flop histograms, and tools/gen_ochs.py end to end -- bit for bit against the numpy restatement tests/np_ochs.py.  No tolerance
anywhere.  Every test prints its figures on a line that starts with OCHS (pytest -s)."""
import itertools
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
from rustsolver_amd.solver import DeviceBuffer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ehs as ne  # noqa: E402
import np_ochs as no  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 0xCDCDCDCD                # what rs_dmemset(0xCD) leaves in every word: -4.3e8, no feature has these bits
BROADWAY = [32, 37, 42, 47, 48]
PAIRED = [0, 1, 22, 35, 49]
ACES = [48, 49, 0, 22, 35]
LOW = [4, 9, 14, 23, 31]
FOUR_FLUSH = [0, 8, 20, 36, 45]
TURN_PAIRED = [0, 1, 22, 35]
ROYAL_DRAW = [32, 36, 40, 44]
FLOP_PAIRED = [0, 1, 20]
FLOP_LAST = [49, 50, 51]
RIVER_BOARDS = [BROADWAY, PAIRED, ACES, LOW, FOUR_FLUSH]
ROUND_CLUSTERS = 2                   # the whole river round: 123 156 254 rows x 2 floats = 1 GB
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_ochs.py")
TOOL_TIMEOUT = 120                   # gen_emd's: a run takes 5.6 s (profiles/ochs.md)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


@pytest.fixture(scope="module")
def table():
    n_actions, tree = rs.build_game_tree(rs.default_flop())
    return rs.create_infosets(n_actions, tree, [4], [1])


@pytest.fixture(scope="module")
def indexers():
    return {nb: ab.HandIndexer([2, nb]) for nb in (3, 4, 5)}


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def report(name, **figures):
    print("OCHS %s: %s" % (name, ", ".join("%s %s" % (k.replace("_", " "), ("%.3f" % v) if isinstance(v, float) else v) for k, v in figures.items())))


def partition(n_clusters):
    """the seeded partition cut to its first n_clusters ranges: the hands of the others are in none"""
    pc = no.seeded_partition()
    return np.where(pc < n_clusters, pc, no.NO_CLUSTER).astype(np.uint8)


def hands_of(board):
    pairs = ne.hole_pairs(board)
    return np.concatenate([pairs, np.tile(np.asarray(board), (len(pairs), 1))], axis=1).astype(np.uint8)


def relabel(cards, perm):
    return [4 * (int(c) >> 2) + perm[int(c) & 3] for c in cards]


def sentinel_buffer(table, indexer, n_clusters):
    rows = indexer.size(1)
    out = ab.RoundHistograms(table, rows, n_clusters, DeviceBuffer(table, rows * n_clusters * 4))
    L.check(L.load().rs_dmemset(table._h, out.ptr, 0xCD, out.nbytes))
    return out


def rows_of(out, idx):
    u, inv = np.unique(idx, return_inverse=True)
    return out.gather(u).view(np.uint32)[inv]


def written_rows(table, out):
    """the rows of a table on the device that are not all sentinel, found on the device: the L2 distance (rs_kmeans_predict, one center) of a row to the row of
    sentinels is +0.0 if and only if every word is the sentinel (test_gpu_ehs_rounds.py).  Only the distances come to the host"""
    center = np.full((1, out.n_bins), SENTINEL, dtype=np.uint32).view(F32)
    dm = DeviceBuffer(table, out.rows * 4)
    L.check(L.load().rs_kmeans_predict(table._h, ab.DIST_L2, out.ptr, out.rows, center.ctypes.data, 1, out.n_bins, None, dm.ptr))
    d = dm.download(F32, out.rows)
    dm.free()
    return np.nonzero(~(d == 0))[0]


def compare_board(got_rows, board, pair_cluster, n_clusters, normalize):
    pairs, want = no.board_features(board, pair_cluster, n_clusters, normalize)
    assert got_rows.shape == want.shape and len(pairs) == {3: 1176, 4: 1128, 5: 1081}[len(board)]
    bad = np.nonzero((got_rows != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, (board, len(bad), pairs[bad[:5]].tolist(), got_rows[bad[:2]].view(F32), want[bad[:2]])
    return want.size


def check_listed(table, indexer, boards, pair_cluster, n_clusters, normalize):
    """listed boards into a sentinel-filled table: their rows are the restatement's, no other row was written -> (cells compared, rows written)"""
    out = sentinel_buffer(table, indexer, n_clusters)
    assert ab.ochs_features(table, indexer, pair_cluster, n_clusters, normalize, boards=boards, out=out) is out
    cells, touched = 0, []
    for board in boards:
        idx = indexer.get_index(hands_of(board)).astype(np.int64)
        cells += compare_board(rows_of(out, idx), board, pair_cluster, n_clusters, normalize)
        touched.append(idx)
    written = written_rows(table, out)
    out.buffer.free()
    assert np.array_equal(written, np.unique(np.concatenate(touched))), "a row of no listed board was written"
    return cells, len(written)


# ---- listed boards ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n_clusters", [1, 3, 8])
def test_river_listed_boards_equal_the_restatement(table, indexers, n_clusters, normalize):
    t0 = time.perf_counter()
    cells, written = check_listed(table, indexers[5], RIVER_BOARDS, partition(n_clusters), n_clusters, normalize)
    report("river listed, %d clusters, normalize %d" % (n_clusters, normalize), rows=5 * 1081, cells=cells, differ=0, rows_written=written, wall_s=time.perf_counter() - t0)


@pytest.mark.parametrize("name,boards", [("turn", [TURN_PAIRED, ROYAL_DRAW]), ("flop", [FLOP_PAIRED, FLOP_LAST])])
def test_turn_and_flop_listed_boards_equal_the_restatement(table, indexers, name, boards):
    t0 = time.perf_counter()
    cells, written = check_listed(table, indexers[len(boards[0])], boards, partition(8), 8, 1)
    report("%s listed, 8 clusters" % name, rows=2 * (1128 if name == "turn" else 1176), cells=cells, differ=0, rows_written=written, wall_s=time.perf_counter() - t0)


@pytest.mark.parametrize("board", [PAIRED, TURN_PAIRED, FLOP_PAIRED], ids=["river", "turn", "flop"])
def test_one_cluster_of_every_pair_is_rs_ehs(table, indexers, board):
    """against pinned code: with every pair in one range and no normalisation the feature is the EHS, bit for bit"""
    t0 = time.perf_counter()
    indexer, hands = indexers[len(board)], hands_of(board)
    out = ab.ochs_features(table, indexer, no.single_cluster(), 1, normalize=False, boards=[board])
    got = rows_of(out, indexer.get_index(hands).astype(np.int64))[:, 0]
    out.buffer.free()
    want = bits(ab.ehs(table, hands))
    differ = int((got != want).sum())
    report("one cluster against rs_ehs, %d board cards" % len(board), hands=len(hands), differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0


# ---- the whole rounds ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def river_round(table, indexers):
    """boards = None at 2 clusters into a sentinel-filled table (1 GB), once; it stays on the device"""
    out = sentinel_buffer(table, indexers[5], ROUND_CLUSTERS)
    t0 = time.perf_counter()
    ab.ochs_features(table, indexers[5], partition(ROUND_CLUSTERS), ROUND_CLUSTERS, True, out=out)
    report("river_round fixture", classes=134459, rows=out.rows, clusters=ROUND_CLUSTERS, sweep_s=time.perf_counter() - t0)
    yield out
    out.buffer.free()


def river_samples():
    rng = np.random.Generator(np.random.PCG64(2025))
    total = 2598960
    numbers = [0, total - 1, ne.board_number(PAIRED), ne.board_number(ACES)] + rng.integers(0, total, size=3).tolist()
    return [(n, ne.board_by_number(5, n)) for n in numbers]


def test_river_round_sampled_boards_equal_the_restatement(river_round, indexers):
    t0, cells = time.perf_counter(), 0
    samples = river_samples()
    assert samples[0][1] == [0, 1, 2, 3, 4] and samples[1][1] == [47, 48, 49, 50, 51] and len({n for n, _ in samples}) == 7
    assert sorted(samples[2][1]) == sorted(PAIRED) and sorted(samples[3][1]) == sorted(ACES)
    for _, board in samples:
        idx = indexers[5].get_index(hands_of(board)).astype(np.int64)
        cells += compare_board(rows_of(river_round, idx), board, partition(ROUND_CLUSTERS), ROUND_CLUSTERS, True)
    report("river sampled boards", boards=[n for n, _ in samples], rows=7 * 1081, cells=cells, differ=0, wall_s=time.perf_counter() - t0)


def test_river_round_leaves_no_row_unwritten(table, river_round):
    t0 = time.perf_counter()
    assert river_round.rows == 123156254
    written = written_rows(table, river_round)
    report("river every row", rows=river_round.rows, rows_written=len(written), wall_s=time.perf_counter() - t0)
    assert len(written) == river_round.rows


def test_a_relabelled_river_board_listed_alone_writes_what_the_round_holds(table, river_round, indexers):
    t0 = time.perf_counter()
    twin = relabel(PAIRED, [2, 0, 3, 1])[::-1][:2] + relabel(PAIRED, [2, 0, 3, 1])[:3]      # relabelled, and its cards out of order
    assert sorted(twin) != sorted(PAIRED) and sorted(c >> 2 for c in twin) == sorted(c >> 2 for c in PAIRED) and twin != sorted(twin)
    out = sentinel_buffer(table, indexers[5], ROUND_CLUSTERS)
    ab.ochs_features(table, indexers[5], partition(ROUND_CLUSTERS), ROUND_CLUSTERS, True, boards=[twin], out=out)
    idx = np.unique(indexers[5].get_index(hands_of(twin)).astype(np.int64))
    assert (idx == np.unique(indexers[5].get_index(hands_of(PAIRED)).astype(np.int64))).all()
    differ = int((rows_of(out, idx) != rows_of(river_round, idx)).any(axis=1).sum())
    written = written_rows(table, out)
    out.buffer.free()
    report("river relabelled board", board=twin, rows=len(idx), differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0 and np.array_equal(written, idx)


def test_turn_round_equals_every_board_listed(table, indexers):
    """boards = NULL (one board per suit-isomorphism class) against all 270 725 turn boards listed, at 1 cluster: equal tables, no row left out"""
    t0 = time.perf_counter()
    boards = ne.round_boards(4)
    assert boards.shape == (270725, 4)
    pc = partition(1)
    a, b = sentinel_buffer(table, indexers[4], 1), sentinel_buffer(table, indexers[4], 1)
    t1 = time.perf_counter()
    ab.ochs_features(table, indexers[4], pc, 1, True, out=a)
    t2 = time.perf_counter()
    ab.ochs_features(table, indexers[4], pc, 1, True, boards=boards, out=b)
    t3 = time.perf_counter()
    x, y = a.download().view(np.uint32), b.download().view(np.uint32)
    a.buffer.free()
    b.buffer.free()
    differ, unwritten = int((x != y).sum()), int((x == SENTINEL).sum())
    report("turn NULL against listed", boards=len(boards), rows=len(x), differ=differ, unwritten=unwritten, null_sweep_s=t2 - t1, listed_sweep_s=t3 - t2,
           wall_s=time.perf_counter() - t0)
    assert differ == 0 and unwritten == 0 and len(x) == 13960050


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing_and_hold_nothing(table, indexers):
    lib = L.load()
    out = sentinel_buffer(table, indexers[3], 8)
    counts = DeviceBuffer(table, 1326 * 64 * 4)
    L.check(lib.rs_dmemset(table._h, counts.ptr, 0xCD, counts.nbytes))
    db, n = ab._card_rows(table, np.array([FLOP_PAIRED], dtype=np.uint8), 3)
    ab.ochs_features(table, indexers[3], partition(8), 8, boards=[FLOP_LAST]).buffer.free()      # the indexer's tables are on the device from here on
    good = partition(8)
    wrong = good.copy()
    wrong[700] = 8
    low = partition(3).copy()
    low[5] = 3
    other = [ab.HandIndexer([2]), ab.HandIndexer([2, 3, 1]), ab.HandIndexer([3, 2]), ab.HandIndexer([2, 2])]
    before = lib.rs_device_held_bytes()

    def features(indexer, pc, n_clusters, out_ptr, boards=db.ptr, n_boards=n):
        return lib.rs_ochs_round_features(table._h, indexer._h, pc.ctypes.data, n_clusters, 1, boards, n_boards, out_ptr)

    cases = [features(ix, good, 8, out.ptr) for ix in other]
    cases += [features(indexers[3], good, bad, out.ptr) for bad in (0, -1, 9)]
    cases += [features(indexers[3], wrong, 8, out.ptr), features(indexers[3], low, 3, out.ptr), features(indexers[3], good, 7, out.ptr)]
    cases += [features(indexers[3], good, 8, None), features(indexers[3], good, 8, None, None, 0)]
    cases += [lib.rs_ehs_preflop_counts(table._h, bad, db.ptr, n, counts.ptr) for bad in (0, -3, ab.EHS_MAX_BINS + 1)]
    cases += [lib.rs_ehs_preflop_counts(table._h, 20, db.ptr, n, None), lib.rs_ehs_preflop_counts(table._h, 20, None, 0, None)]
    assert cases == [L.ERR_INVALID] * len(cases) and len(cases) == 17, cases
    assert lib.rs_device_held_bytes() == before
    assert len(written_rows(table, out)) == 0 and (counts.download(np.uint32, 1326 * 64) == SENTINEL).all()
    # an empty list is no work: fine, and nothing is written
    assert features(indexers[3], good, 8, None, db.ptr, 0) == L.OK and len(written_rows(table, out)) == 0
    # a bad board in a list is reported, the others are done
    listed = np.array([FLOP_PAIRED, [7, 7, 30], FLOP_LAST, [3, 52, 9]], dtype=np.uint8)
    with pytest.raises(rs.RsError) as e:
        ab.ochs_features(table, indexers[3], good, 8, boards=listed, out=out)
    assert e.value.code == L.ERR_INVALID and "repeats a card" in str(e.value)
    idx = [indexers[3].get_index(hands_of(b)).astype(np.int64) for b in (FLOP_PAIRED, FLOP_LAST)]
    for board, at in zip((FLOP_PAIRED, FLOP_LAST), idx):
        compare_board(rows_of(out, at), board, good, 8, True)
    assert np.array_equal(written_rows(table, out), np.unique(np.concatenate(idx)))
    with pytest.raises(rs.RsError) as e:
        ab.preflop_counts(table, 20, boards=listed)
    assert e.value.code == L.ERR_INVALID and lib.rs_device_held_bytes() == before
    out.buffer.free()
    counts.free()


# ---- the preflop counts -------------------------------------------------------------------------------------------------------------------------------------------
def test_preflop_counts_of_listed_flops_equal_the_restatement(table):
    t0 = time.perf_counter()
    flops = [FLOP_PAIRED, FLOP_LAST]
    got = ab.preflop_counts(table, 20, boards=flops)
    want = no.preflop_counts(flops, 20)
    assert got.dtype == np.uint32 and got.shape == want.shape == (1326, 20)
    differ = int((got.astype(np.int64) != want).sum())
    report("preflop listed", flops=2, cells=want.size, differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0


@pytest.mark.parametrize("n_bins", [1, 64])
def test_preflop_counts_of_listed_flops_equal_the_device_histograms_of_those_flops(table, indexers, n_bins):
    """test_the_preflop_counts_of_two_listed_flops (test_ochs_cpu.py) on the device: the two kernels that share one histogram body, each through its own last step.
    The rows of rs_ehs_round_histograms for the two flops (pinned at these bin counts by test_gpu_ehs_rounds.py), as counts, placed by each hand's hole cards and
    summed over the flops, are the preflop counts cell for cell.  64 bins is the 163 328-byte launch; 1 bin leaves the last uint16 cell of the histogram unpaired"""
    t0 = time.perf_counter()
    flops = [FLOP_PAIRED, FLOP_LAST]
    got = ab.preflop_counts(table, n_bins, boards=flops)
    hist = ab.round_histograms(table, indexers[3], n_bins, boards=flops)
    want = np.zeros((1326, n_bins), dtype=np.int64)
    for flop in flops:
        hands = hands_of(flop).astype(np.int64)
        k = ne.counts_of_words(rows_of(hist, indexers[3].get_index(hands.astype(np.uint8)).astype(np.int64)), 1081).astype(np.int64)
        assert k.shape == (1176, n_bins) and k.min() >= 0 and (k.sum(axis=1) == 1081).all()
        want[no.pair_index(hands[:, 0], hands[:, 1])] += k      # the 1176 hole pairs of a flop are 1176 different rows
    hist.buffer.free()
    assert got.dtype == np.uint32 and got.shape == want.shape and int(want.sum()) == 2 * 1176 * 1081
    differ = int((got.astype(np.int64) != want).sum())
    report("preflop against the device's flop histograms, %d bins" % n_bins, flops=2, cells=want.size, differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0


@pytest.fixture(scope="module")
def all_flops_35(table):
    t0 = time.perf_counter()
    counts = ab.preflop_counts(table, 35)
    report("preflop all flops fixture", bins=35, sweep_s=time.perf_counter() - t0)
    counts.setflags(write=False)
    return counts


def test_preflop_counts_over_all_flops_add_up(all_flops_35):
    assert all_flops_35.shape == (1326, 35)
    assert (all_flops_35.sum(axis=1, dtype=np.int64) == 21187600).all() and (all_flops_35 % 10 == 0).all()


def test_preflop_class_sums_equal_a_fold_of_the_flop_histograms(table, indexers, all_flops_35):
    """Independent of the new kernel: every canonical flop row of rs_ehs_round_histograms (pinned by test_gpu_ehs_rounds.py), as counts, times the number of hands it
    stands for, added to the preflop class of its hole cards.  A row stands for 24 / (the suit permutations that fix its representative hand) hands"""
    t0 = time.perf_counter()
    flop = indexers[3]
    hist = ab.round_histograms(table, flop, 35)
    k = ne.counts_of_words(hist.download().view(np.uint32), 1081).astype(np.int64)
    hist.buffer.free()
    assert k.min() >= 0 and (k.sum(axis=1) == 1081).all()
    hands = flop.get_hand(1, np.arange(flop.size(1), dtype=np.uint64)).astype(np.int64)

    def as_sets(h):      # a hand is its set of hole cards and its set of board cards
        return np.sort(h[:, :2], axis=1), np.sort(h[:, 2:], axis=1)

    hole, board = as_sets(hands)
    fixed = np.zeros(len(hands), dtype=np.int64)
    for perm in itertools.permutations(range(4)):
        h2, b2 = as_sets(4 * (hands >> 2) + np.asarray(perm)[hands & 3])
        fixed += (h2 == hole).all(axis=1) & (b2 == board).all(axis=1)
    orbit = 24 // fixed
    assert (24 % fixed == 0).all() and int(orbit.sum()) == 1326 * 19600          # every hole pair with every flop off it
    two = ab.HandIndexer([2])
    cls = two.get_index(hands[:, :2].astype(np.uint8)).astype(np.int64)
    fold = np.stack([np.bincount(cls, weights=(k[:, b] * orbit).astype(np.float64), minlength=169) for b in range(35)], axis=1).astype(np.int64)
    pair_cls = two.get_index(no.hole_cards().astype(np.uint8)).astype(np.int64)
    sums = np.zeros((169, 35), dtype=np.int64)
    np.add.at(sums, pair_cls, all_flops_35.astype(np.int64))
    differ = int((sums != fold).sum())
    report("preflop fold", rows=len(hands), classes=169, differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0
    # and the histograms the opponent ranges are clustered by are these sums over the class sizes
    got = ab.preflop_histograms(table, 35)
    n_pairs = np.bincount(pair_cls, minlength=169)
    want = (sums.astype(np.float64) / (n_pairs * 21187600).astype(np.float64)[:, None]).astype(F32)
    assert got.shape == (169, 35) and (bits(got) == bits(want)).all()


def test_opponent_clusters_are_a_partition_by_class_in_ascending_strength(table, all_flops_35):
    t0 = time.perf_counter()
    pc = ab.opponent_clusters(table, 8, 35, seed=1)
    assert pc.shape == (1326,) and pc.dtype == np.uint8 and (pc == ab.opponent_clusters(table, 8, 35, seed=1)).all()
    cls = no.preflop_classes()[1]
    assert len(set(zip(cls.tolist(), pc.tolist()))) == 169 and set(pc.tolist()) <= set(range(8))
    bins = np.arange(35, dtype=np.float64)
    means = []
    for c in sorted(set(pc.tolist())):
        total = all_flops_35[pc == c].astype(np.int64).sum(axis=0)
        means.append(float(np.dot(bins, total.astype(np.float64)) / np.float64(total.sum())))
    report("opponent clusters", used=len(means), mean_bins=[round(m, 3) for m in means], wall_s=time.perf_counter() - t0)
    assert means == sorted(means) and len(means) > 1
    assert pc[no.pair_index(48, 49)] == max(pc)      # AA is in the strongest range


# ---- the tool, end to end -----------------------------------------------------------------------------------------------------------------------------------------
def test_gen_ochs_gives_the_same_river_bucket_file_twice(tmp_path, table, indexers):
    t0 = time.perf_counter()
    files, lines, seconds = [tmp_path / "a.dat", tmp_path / "b.dat"], [], []
    for path in files:      # one fresh child at a time; the second only after the first came back clean
        t1 = time.perf_counter()
        r = subprocess.run([sys.executable, TOOL, "--round", "3", "--clusters", "64", "--opp-clusters", "8", "--seed", "7", "--out", str(path)], capture_output=True,
                           text=True, timeout=TOOL_TIMEOUT)
        seconds.append(time.perf_counter() - t1)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    river = indexers[5]
    rows = river.size(1)
    assert rows == 123156254
    assert files[0].read_bytes() == files[1].read_bytes()
    for line in lines:
        assert line["rows"] == rows and line["clusters"] == 64 and line["seed"] == 7 and line["opp_clusters"] == 8 and sum(line["range_sizes"]) == 1326
    assert lines[0]["xor"] == lines[1]["xor"] and lines[0]["inertia"] == lines[1]["inertia"]
    clusters = ab.read_cluster_file(str(files[0]))
    assert clusters.dtype == np.uint32 and clusters.shape == (rows,) and int(clusters.max()) < 64
    assert len(np.unique(clusters)) == lines[0]["used_clusters"] > 1
    # CardAbstraction reads it as the river's bucket file
    mask = sum(1 << c for c in PAIRED)
    hole = ab.random_range(mask)
    card_abs = ab.CardAbstraction.init([hole, hole], mask, ab.RIVER, clusters)
    assert card_abs.index_size() == rows and 1 < card_abs.get_size(0) <= 64
    # hands with bit-equal feature rows lie in one cluster, whichever rows they have.  The rows are the restatement's under the partition of a run of the library
    # with the tool's seed -- what the tool clustered
    pc = ab.opponent_clusters(table, 8, 35, seed=7)
    by_features = {}
    for board in (PAIRED, BROADWAY, LOW):
        pairs, f = no.board_features(board, pc, 8, True)
        for row, fb in zip(river.get_index(hands_of(board)).astype(np.int64).tolist(), bits(f)):
            by_features.setdefault(fb.tobytes(), set()).add(row)
    shared = [sorted(r) for r in by_features.values() if len(r) > 1]
    assert len(shared) >= 5
    split = [r for r in shared if len(set(clusters[r].tolist())) != 1]
    report("gen_ochs twice", tool_runs_s=seconds, features_shared_by_several_rows=len(shared), rows_in_them=sum(len(r) for r in shared), split_between_clusters=len(split),
           used_clusters=lines[0]["used_clusters"], wall_s=time.perf_counter() - t0)
    assert not split, split[:3]
