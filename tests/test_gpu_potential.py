"""GPU (-m gpu): the potential-aware abstraction -- rs_next_round_histograms (listed boards, suit relabelling, the whole flop and turn rounds, the refusals),
rs_pa_predict and rs_pa_fit on synthetic rows, ab.ground_distances and tools/gen_potential.py end to end -- bit for bit against the numpy restatement
tests/np_potential.py.  No tolerance anywhere.  Every test prints its figures on a line that starts with POTENTIAL (pytest -s)."""
import ctypes as C
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
import np_potential as npp  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
W = ab.PA_ROW_WORDS
SENTINEL = 0xCDCDCDCD                # what rs_dmemset(0xCD) leaves in every word: no row word has these bits (a bucket is below 8192)
FLOPS = [[0, 1, 20], [49, 50, 51], [2, 18, 46]]      # paired, the last one, monotone
TURNS = [[0, 1, 22, 35], [32, 36, 40, 44]]
RIVER_NEXT = 300                     # buckets of the synthetic river file
TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_potential.py")
TOOL_TIMEOUT = 120                   # the other tool tests' limit


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


@pytest.fixture(scope="module")
def river_file(table, indexers):
    """the synthetic 123 M-entry river bucket file at RIVER_NEXT buckets, built and uploaded once"""
    t0 = time.perf_counter()
    buf = DeviceBuffer.from_numpy(table, npp.synthetic_buckets(indexers[5].size(1), RIVER_NEXT))
    report("river_file fixture", entries=indexers[5].size(1), n_next=RIVER_NEXT, build_and_upload_s=time.perf_counter() - t0)
    yield buf
    buf.free()


def report(name, **figures):
    print("POTENTIAL %s: %s" % (name, ", ".join("%s %s" % (k.replace("_", " "), ("%.3f" % v) if isinstance(v, float) else v) for k, v in figures.items())))


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def hands_of(board):
    pairs = ne.hole_pairs(board)
    return np.concatenate([pairs, np.tile(np.asarray(board), (len(pairs), 1))], axis=1).astype(np.uint8)


def relabel(cards, perm):
    return [4 * (int(c) >> 2) + perm[int(c) & 3] for c in cards]


def sentinel_rows(table, indexer):
    rows = indexer.size(1)
    out = ab.SparseRows(table, rows, 52 - indexer.n_cards(1), DeviceBuffer(table, rows * W * 4))
    L.check(L.load().rs_dmemset(table._h, out.ptr, 0xCD, out.nbytes))
    return out


def rows_of(out, idx):
    u, inv = np.unique(idx, return_inverse=True)
    return out.gather(u)[inv]


def written_rows(table, out):
    """the rows of a table on the device that are not all sentinel, found on the device: the L2 distance (rs_kmeans_predict, one centre, the words read as floats) of a
    row to the row of sentinels is +0.0 if and only if every word is the sentinel (test_gpu_ochs.py).  Only the distances come to the host"""
    center = np.full((1, W), SENTINEL, dtype=np.uint32).view(F32)
    dm = DeviceBuffer(table, out.rows * 4)
    L.check(L.load().rs_kmeans_predict(table._h, ab.DIST_L2, out.ptr, out.rows, center.ctypes.data, 1, W, None, dm.ptr))
    d = dm.download(F32, out.rows)
    dm.free()
    return np.nonzero(~(d == 0))[0]


def restated(indexers, hands, n_next):
    nb = hands.shape[1] - 2
    return npp.hand_rows(indexers[nb + 1], hands, lambda idx: npp.synthetic_bucket_at(idx, n_next), n_next)


def check_listed(table, indexers, boards, next_buckets, n_next):
    """listed boards into a sentinel-filled table: their rows are the restatement's, no other row was written -> (rows compared, rows written)"""
    nb = len(boards[0])
    out = sentinel_rows(table, indexers[nb])
    assert ab.next_round_histograms(table, indexers[nb], indexers[nb + 1], next_buckets, n_next, boards=boards, out=out) is out
    compared, touched = 0, []
    for board in boards:
        hands = hands_of(board)
        idx = indexers[nb].get_index(hands).astype(np.int64)
        got, want = rows_of(out, idx), restated(indexers, hands, n_next)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (board, len(bad), hands[bad[:3]].tolist(), got[bad[:2]], want[bad[:2]])
        assert all(npp.well_formed(r, n_next, 50 - nb) for r in got[:50])
        compared += len(hands)
        touched.append(idx)
    written = written_rows(table, out)
    out.buffer.free()
    assert np.array_equal(written, np.unique(np.concatenate(touched))), "a row of no listed board was written"
    return compared, len(written)


# ---- the histogram kernel: listed boards ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_next", [1, 2, 300, 8192])
def test_listed_flops_equal_the_restatement(table, indexers, n_next):
    t0 = time.perf_counter()
    turn_file = npp.synthetic_buckets(indexers[4].size(1), n_next)
    compared, written = check_listed(table, indexers, FLOPS, turn_file, n_next)
    report("flop listed, %d next buckets" % n_next, rows=compared, differ=0, rows_written=written, wall_s=time.perf_counter() - t0)
    assert compared == 3 * 1176


def test_listed_turn_boards_equal_the_restatement(table, indexers, river_file):
    t0 = time.perf_counter()
    compared, written = check_listed(table, indexers, TURNS, river_file, RIVER_NEXT)
    report("turn listed", rows=compared, differ=0, rows_written=written, wall_s=time.perf_counter() - t0)
    assert compared == 2 * 1128


@pytest.mark.parametrize("board", [FLOPS[0], TURNS[0]], ids=["flop", "turn"])
def test_a_relabelled_board_writes_the_same_rows(table, indexers, river_file, board):
    t0 = time.perf_counter()
    nb = len(board)
    twin = relabel(board, [2, 0, 3, 1])[::-1]                                # relabelled, and its cards out of order
    assert sorted(twin) != sorted(board) and sorted(c >> 2 for c in twin) == sorted(c >> 2 for c in board)
    n_next = 300 if nb == 3 else RIVER_NEXT
    file = npp.synthetic_buckets(indexers[4].size(1), n_next) if nb == 3 else river_file
    a, b = sentinel_rows(table, indexers[nb]), sentinel_rows(table, indexers[nb])
    ab.next_round_histograms(table, indexers[nb], indexers[nb + 1], file, n_next, boards=[board], out=a)
    ab.next_round_histograms(table, indexers[nb], indexers[nb + 1], file, n_next, boards=[twin], out=b)
    idx = np.unique(indexers[nb].get_index(hands_of(board)).astype(np.int64))
    assert (idx == np.unique(indexers[nb].get_index(hands_of(twin)).astype(np.int64))).all()
    x, y = rows_of(a, idx), rows_of(b, idx)
    wa, wb = written_rows(table, a), written_rows(table, b)
    a.buffer.free()
    b.buffer.free()
    differ = int((x != y).any(axis=1).sum())
    report("relabelled board, %d cards" % nb, board=twin, rows=len(idx), differ=differ, wall_s=time.perf_counter() - t0)
    assert differ == 0 and (x != SENTINEL).all() and np.array_equal(wa, idx) and np.array_equal(wb, idx)


# ---- the whole rounds -----------------------------------------------------------------------------------------------------------------------------------------------
def check_round(table, indexers, nb, file, n_next, slice_rows=1 << 21):
    indexer, n_draws = indexers[nb], 50 - nb
    out = sentinel_rows(table, indexer)
    t0 = time.perf_counter()
    ab.next_round_histograms(table, indexer, indexers[nb + 1], file, n_next, out=out)
    sweep = time.perf_counter() - t0
    written = len(written_rows(table, out))
    rng = np.random.Generator(np.random.PCG64(2014 + nb))
    idx = np.unique(np.concatenate([[0, out.rows - 1], rng.integers(0, out.rows, size=20000)])).astype(np.int64)
    taken, wrong_sum = np.empty((len(idx), W), dtype=np.uint32), 0
    for first in range(0, out.rows, slice_rows):      # one pass over the table in slices: the turn round is 2.7 GB
        x = out.download(first, min(slice_rows, out.rows - first))
        wrong_sum += int(((x & 255).sum(axis=1) != n_draws).sum())
        lo, hi = np.searchsorted(idx, first), np.searchsorted(idx, first + slice_rows)
        taken[lo:hi] = x[idx[lo:hi] - first]
    out.buffer.free()
    want = restated(indexers, indexer.get_hand(1, idx.astype(np.uint64)), n_next)
    differ = int((taken != want).any(axis=1).sum())
    return {"rows": out.rows, "rows_written": written, "rows_with_a_wrong_sum": wrong_sum, "sampled": len(idx), "differ": differ, "sweep_s": sweep}


def test_the_whole_flop_round(table, indexers):
    t0 = time.perf_counter()
    f = check_round(table, indexers, 3, npp.synthetic_buckets(indexers[4].size(1), 300), 300)
    report("flop round", wall_s=time.perf_counter() - t0, **f)
    assert f["rows"] == f["rows_written"] == 1286792 and f["rows_with_a_wrong_sum"] == 0 and f["differ"] == 0 and f["sampled"] > 19000


def test_the_whole_turn_round(table, indexers, river_file):
    t0 = time.perf_counter()
    f = check_round(table, indexers, 4, river_file, RIVER_NEXT)
    report("turn round", wall_s=time.perf_counter() - t0, **f)
    assert f["rows"] == f["rows_written"] == 13960050 and f["rows_with_a_wrong_sum"] == 0 and f["differ"] == 0 and f["sampled"] > 19000


# ---- refusals and reports -------------------------------------------------------------------------------------------------------------------------------------------
def test_histogram_refusals_touch_nothing_and_bad_boards_are_reported(table, indexers):
    lib = L.load()
    out = sentinel_rows(table, indexers[3])
    file = DeviceBuffer.from_numpy(table, npp.synthetic_buckets(indexers[4].size(1), 300))
    db, n = ab._card_rows(table, np.array([FLOPS[0]], dtype=np.uint8), 3)
    ab.next_round_histograms(table, indexers[3], indexers[4], file, 300, boards=[FLOPS[1]]).buffer.free()      # the indexers' tables are on the device from here on
    before = lib.rs_device_held_bytes()

    def rows(ix, nx, n_next, buckets=file.ptr, boards=db.ptr, n_boards=n, out_ptr=out.ptr):
        return lib.rs_next_round_histograms(table._h, ix._h if ix else None, nx._h if nx else None, buckets, n_next, boards, n_boards, out_ptr)

    two = ab.HandIndexer([2])
    cases = [rows(indexers[3], indexers[5], 300), rows(indexers[4], indexers[4], 300), rows(indexers[5], indexers[5], 300), rows(indexers[4], indexers[3], 300),
             rows(two, indexers[4], 300), rows(indexers[3], ab.HandIndexer([2, 3, 1]), 300), rows(None, indexers[4], 300), rows(indexers[3], None, 300)]
    cases += [rows(indexers[3], indexers[4], bad) for bad in (0, -1, ab.PA_MAX_NEXT + 1)]
    cases += [rows(indexers[3], indexers[4], 300, buckets=None), rows(indexers[3], indexers[4], 300, out_ptr=None),
              rows(indexers[3], indexers[4], 300, boards=None, n_boards=0, out_ptr=None)]
    assert cases == [L.ERR_INVALID] * len(cases) and len(cases) == 14, cases
    assert lib.rs_device_held_bytes() == before and len(written_rows(table, out)) == 0
    assert rows(indexers[3], indexers[4], 300, n_boards=0, out_ptr=None) == L.OK and len(written_rows(table, out)) == 0      # an empty list is no work
    # a bad board in a list is reported, the others are done
    listed = np.array([FLOPS[0], [7, 7, 30], FLOPS[1], [3, 52, 9]], dtype=np.uint8)
    with pytest.raises(rs.RsError) as e:
        ab.next_round_histograms(table, indexers[3], indexers[4], file, 300, boards=listed, out=out)
    assert e.value.code == L.ERR_INVALID and "repeats a card" in str(e.value)
    idx = [indexers[3].get_index(hands_of(b)).astype(np.int64) for b in (FLOPS[0], FLOPS[1])]
    for board, at in zip((FLOPS[0], FLOPS[1]), idx):
        assert (rows_of(out, at) == restated(indexers, hands_of(board), 300)).all()
    assert np.array_equal(written_rows(table, out), np.unique(np.concatenate(idx)))
    out.buffer.free()
    # a bucket that is not below n_next is reported; the hands that reach it keep their rows, the others are done
    out = sentinel_rows(table, indexers[3])
    with pytest.raises(rs.RsError) as e:
        ab.next_round_histograms(table, indexers[3], indexers[4], file, 299, boards=[FLOPS[2]], out=out)
    assert e.value.code == L.ERR_INVALID and "n_next" in str(e.value)
    hands = hands_of(FLOPS[2])
    at = indexers[3].get_index(hands).astype(np.int64)
    want = restated(indexers, hands, 300)
    reach = ((want >> 8) == 299).any(axis=1)
    assert 50 < reach.sum() < len(hands) - 50
    got = rows_of(out, at)
    clean = ~np.isin(at, at[reach])                                              # two hands of the board may share a row
    assert (got[clean] == want[clean]).all() and (got[reach] == SENTINEL).all()
    assert np.array_equal(written_rows(table, out), np.unique(at[clean]))
    out.buffer.free()
    file.free()


# ---- rs_pa_predict --------------------------------------------------------------------------------------------------------------------------------------------------
def device_rows(table, rows, n_draws):
    return ab.SparseRows(table, len(rows), n_draws, DeviceBuffer.from_numpy(table, np.ascontiguousarray(rows, dtype=np.uint32)))


def grounds(rng, n_next):
    return {"ties": npp.tie_ground(n_next), "duplicates": npp.random_ground(rng, n_next, duplicates=3)}


def make_means(rng, rows, n_means, n_next, n_draws):
    """means of mass 1 (points, means of two points), below 1 and above 1; with more than one, mean 1 is a copy of mean 0, so that the first of the two wins"""
    dense = npp.dense(rows, n_next, n_draws)
    out = np.zeros((n_means, n_next), dtype=F32)
    for k in range(n_means):
        a, b = dense[rng.integers(0, len(rows))], dense[rng.integers(0, len(rows))]
        kind = k % 4
        out[k] = a if kind == 0 else ((a.astype(np.float64) + b) / 2).astype(F32) if kind == 1 else a * F32(0.5) if kind == 2 else (a + b) * F32(0.75)
    if n_means > 1:
        out[1] = out[0]
    return out


PREDICT_CASES = [      # n rows, means, next buckets, ground, draws, d_sel
    (1, 1, 1, "ties", 47, False),
    (63, 2, 2, "ties", 46, False),
    (64, 65, 3, "duplicates", 47, True),
    (65, 2, 65, "duplicates", 46, False),
    (65, 65, 65, "ties", 47, True),
    (300, 2, 300, "ties", 47, True),
    (300, 65, 3, "ties", 46, False),
    (300, 1, 2, "duplicates", 47, False),
]


@pytest.mark.parametrize("n,n_means,n_next,ground,n_draws,use_sel", PREDICT_CASES)
def test_predict_equals_the_restatement(table, n, n_means, n_next, ground, n_draws, use_sel):
    t0 = time.perf_counter()
    rng = np.random.Generator(np.random.PCG64(n * 1000 + n_means * 10 + n_next))
    g = grounds(rng, n_next)[ground]
    rows = npp.random_rows(rng, n, n_next, n_draws)
    means = make_means(rng, rows, n_means, n_next, n_draws)
    sel = rng.integers(0, n, size=n + 7).astype(np.uint32) if use_sel else None      # with repeats
    data = rows if sel is None else rows[sel]
    want_c, want_d = npp.predict(data, means, g, n_draws)
    dr = device_rows(table, rows, n_draws)
    got_c, got_d = ab.PotentialKmeans(table, dr, g).predict(means, sel=sel)
    dr.buffer.free()
    differ = int((got_c != want_c).sum() + (bits(got_d) != bits(want_d)).sum())
    report("predict n %d, means %d, next %d, %s, draws %d, sel %s" % (n, n_means, n_next, ground, n_draws, use_sel), data=len(data), differ=differ,
           second_of_two_equal_means_chosen=int((got_c == 1).sum()) if n_means > 1 else 0, wall_s=time.perf_counter() - t0)
    assert differ == 0 and got_c.dtype == np.uint32 and len(got_c) == len(data)
    if n_means > 1:
        assert not (got_c == 1).any()


def test_predict_reports_a_malformed_row_and_does_the_others(table):
    rng = np.random.Generator(np.random.PCG64(77))
    n_next, n_draws = 65, 47
    g = npp.tie_ground(n_next)
    rows = npp.random_rows(rng, 70, n_next, n_draws)
    means = make_means(rng, rows, 5, n_next, n_draws)
    want_c, want_d = npp.predict(rows, means, g, n_draws)
    lib = L.load()
    for name, bad in (("not ascending", npp.pack_row([9, 4], [20, 27])), ("a bucket past n_next", npp.pack_row([4, 65], [20, 27])),
                      ("a count of 0 ahead of a used word", np.concatenate([[4 << 8 | 20, 6 << 8, 9 << 8 | 27], np.zeros(45)]).astype(np.uint32)),
                      ("counts short of n_draws", npp.pack_row([4, 9], [20, 26])), ("no entry", np.zeros(48, dtype=np.uint32))):
        x = rows.copy()
        x[33] = bad
        dr = device_rows(table, x, n_draws)
        km = ab.PotentialKmeans(table, dr, g)
        dc, dm = DeviceBuffer(table, 70 * 4), DeviceBuffer(table, 70 * 4)
        for b in (dc, dm):
            L.check(lib.rs_dmemset(table._h, b.ptr, 0xCD, b.nbytes))
        rc = lib.rs_pa_predict(table._h, km._h, dr.ptr, None, 70, n_draws, means.ctypes.data, 5, dc.ptr, dm.ptr)
        got_c, got_d = dc.download(np.uint32, 70), dm.download(np.uint32, 70)
        for b in (dc, dm, dr.buffer):
            b.free()
        assert rc == L.ERR_INVALID, name
        ok = np.arange(70) != 33
        assert got_c[33] == SENTINEL and got_d[33] == SENTINEL, name
        assert (got_c[ok] == want_c[ok]).all() and (got_d[ok] == bits(want_d)[ok]).all(), name


def test_predict_and_fit_refusals(table):
    lib = L.load()
    rng = np.random.Generator(np.random.PCG64(3))
    rows = npp.random_rows(rng, 10, 7, 47)
    dr = device_rows(table, rows, 47)
    km = ab.PotentialKmeans(table, dr, npp.tie_ground(7))
    host_only = ab.PotentialKmeans(None, dr, npp.tie_ground(7))
    means = npp.dense(rows[:2], 7, 47)
    dc = DeviceBuffer(table, 40)
    changed, ran = np.zeros(3, dtype=np.uint32), C.c_int(-1)
    nan = means.copy()
    nan[1, 2] = np.nan

    def predict(metric=km._h, rows_ptr=dr.ptr, n=10, n_draws=47, m=means, n_means=2):
        return lib.rs_pa_predict(table._h, metric, rows_ptr, None, n, n_draws, m.ctypes.data if m is not None else None, n_means, dc.ptr, None)

    def fit(n=10, iterations=3, ch=changed.ctypes.data, m=means.copy()):
        return lib.rs_pa_fit(table._h, km._h, dr.ptr, None, n, 47, m.ctypes.data, 2, iterations, dc.ptr, None, ch, C.byref(ran))

    cases = [predict(metric=None), predict(metric=host_only._h), predict(rows_ptr=None), predict(n_draws=0), predict(n_draws=48), predict(m=None), predict(n_means=0),
             predict(m=nan), predict(m=-means), fit(n=0), fit(iterations=0), fit(ch=None), fit(m=nan)]
    assert cases == [L.ERR_INVALID] * len(cases), cases
    assert predict(n=0) == L.OK
    dr.buffer.free()
    dc.free()


# ---- rs_pa_fit ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_three_iterations_equal_the_restatement_and_an_empty_cluster_keeps_its_mean(table):
    t0 = time.perf_counter()
    rng = np.random.Generator(np.random.PCG64(300))
    n_next, n_draws = 24, 47
    g = npp.tie_ground(n_next)
    rows = np.stack([npp.random_row(rng, 16, n_draws, int(s)) for s in rng.integers(1, 17, size=300)])      # every row lives on buckets 0..15
    means = npp.dense(rows[rng.choice(300, size=7, replace=False)], n_next, n_draws)
    means[4] = 0
    means[4, 23] = F32(3.0)                                                      # far from every row: it gets no member
    want_c, want_m, want_d, want_ch = npp.fit(rows, means, g, n_draws, 3)
    assert len(want_ch) == 3 and want_ch[0] == 300 and want_ch[2] > 0 and not (want_c == 4).any()
    dr = device_rows(table, rows, n_draws)
    got_c, got_m, got_d, got_ch = ab.PotentialKmeans(table, dr, g).fit(means, iterations=3)
    dr.buffer.free()
    report("fit 300 rows, 7 means, 3 iterations", changed=got_ch.tolist(), clusters_differ=int((got_c != want_c).sum()), means_differ=int((bits(got_m) != bits(want_m)).sum()),
           distances_differ=int((bits(got_d) != bits(want_d)).sum()), wall_s=time.perf_counter() - t0)
    assert got_ch.tolist() == want_ch.tolist() and (got_c == want_c).all() and (bits(got_m) == bits(want_m)).all() and (bits(got_d) == bits(want_d)).all()
    assert (bits(got_m[4]) == bits(means[4])).all() and (bits(got_m[0]) != bits(means[0])).any()


def test_fit_stops_after_an_iteration_without_changes(table):
    t0 = time.perf_counter()
    rng = np.random.Generator(np.random.PCG64(64))
    n_next, n_draws = 7, 46
    g = npp.random_ground(rng, n_next, duplicates=1)
    rows = npp.random_rows(rng, 64, n_next, n_draws)
    sel = rng.integers(0, 64, size=90).astype(np.uint32)
    means = npp.dense(rows[:2], n_next, n_draws)
    want_c, want_m, want_d, want_ch = npp.fit(rows[sel], means, g, n_draws, 20)
    assert len(want_ch) < 20 and want_ch[-1] == 0
    dr = device_rows(table, rows, n_draws)
    got_c, got_m, got_d, got_ch = ab.PotentialKmeans(table, dr, g).fit(means, iterations=20, sel=sel)
    dr.buffer.free()
    report("fit to convergence", iterations_run=len(got_ch), changed=got_ch.tolist(), wall_s=time.perf_counter() - t0)
    assert got_ch.tolist() == want_ch.tolist() and (got_c == want_c).all() and (bits(got_m) == bits(want_m)).all() and (bits(got_d) == bits(want_d)).all()


# ---- ab.ground_distances --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [ab.DIST_EMD, ab.DIST_L2], ids=["emd", "l2"])
def test_ground_distances_equal_the_host_distance_cell_by_cell(table, dist):
    rng = np.random.Generator(np.random.PCG64(9))
    centers = rng.random((9, 20)).astype(F32)
    centers /= centers.sum(axis=1, keepdims=True, dtype=F32)
    centers[5] = centers[2]
    g = ab.ground_distances(table, centers, dist)
    want = np.array([[ab.histogram_distance(centers[i], centers[j], dist) for j in range(9)] for i in range(9)], dtype=F32)
    assert g.shape == (9, 9) and g.dtype == F32 and (bits(g) == bits(want)).all()
    if dist == ab.DIST_L2:      # emd_1d is a heuristic: two equal histograms are not exactly at distance 0 under it
        assert g[2, 5] == 0 and g[5, 2] == 0 and (np.diag(g) == 0).all()


# ---- the tool, end to end -------------------------------------------------------------------------------------------------------------------------------------------
def test_gen_potential_gives_the_same_flop_bucket_file_twice(tmp_path, indexers):
    t0 = time.perf_counter()
    flop, turn = indexers[3], indexers[4]
    rng = np.random.Generator(np.random.PCG64(11))
    ground = npp.random_ground(rng, 64, duplicates=2)
    np.save(tmp_path / "ground.npy", ground)
    ab.write_cluster_file(str(tmp_path / "turn.dat"), npp.synthetic_buckets(turn.size(1), 64))
    files, centers, lines, seconds = [tmp_path / "a.dat", tmp_path / "b.dat"], [tmp_path / "a.npy", tmp_path / "b.npy"], [], []
    for path, cpath in zip(files, centers):      # one fresh child at a time; the second only after the first came back clean
        t1 = time.perf_counter()
        r = subprocess.run([sys.executable, TOOL, "--round", "1", "--clusters", "50", "--next-buckets", str(tmp_path / "turn.dat"), "--ground", str(tmp_path / "ground.npy"),
                            "--seed", "7", "--train-fraction", "20", "--iterations", "3", "--out", str(path), "--centers-out", str(cpath)],
                           capture_output=True, text=True, timeout=TOOL_TIMEOUT)
        seconds.append(time.perf_counter() - t1)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert files[0].read_bytes() == files[1].read_bytes() and centers[0].read_bytes() == centers[1].read_bytes()
    rows = flop.size(1)
    clusters = ab.read_cluster_file(str(files[0]))
    assert clusters.dtype == np.uint32 and clusters.shape == (rows,) and int(clusters.max()) < 50
    for line in lines:
        assert line["rows"] == rows and line["clusters"] == 50 and line["n_next"] == 64 and line["train_rows"] == rows // 20 and 1 <= line["iterations_run"] <= 3
        assert line["changed"][0] == rows // 20
    means = np.load(centers[0])
    assert means.shape == (50, 64) and means.dtype == F32
    idx = np.unique(rng.integers(0, rows, size=5000)).astype(np.int64)
    sampled = npp.hand_rows(turn, flop.get_hand(1, idx.astype(np.uint64)), lambda i: npp.synthetic_bucket_at(i, 64), 64)
    want, _ = npp.predict(sampled, means, ground, 47)
    differ = int((clusters[idx] != want).sum())
    report("gen_potential twice", tool_runs_s=seconds, sampled=len(idx), differ=differ, used_clusters=lines[0]["used_clusters"], changed=lines[0]["changed"],
           wall_s=time.perf_counter() - t0)
    assert differ == 0
    # it refuses to overwrite
    r = subprocess.run([sys.executable, TOOL, "--round", "1", "--clusters", "50", "--next-buckets", str(tmp_path / "turn.dat"), "--ground", str(tmp_path / "ground.npy"),
                        "--out", str(files[0])], capture_output=True, text=True, timeout=TOOL_TIMEOUT)
    assert r.returncode != 0 and "not overwritten" in r.stderr
